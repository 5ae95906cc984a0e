/* cgamd.h -- extended C ABI of the MI355X-native CG solver (gfx950, HIP).
 *
 * Everything here is plain C: pointers, sizes, opaque handles.  No torch types.
 * Device pointers are ordinary `void*` values in the HIP address space (e.g.
 * torch.Tensor.data_ptr()); `stream` arguments are hipStream_t passed as void*
 * (0/NULL = the context's own stream).
 *
 * The API mirrors the reference's operator surface for the CG hot path:
 *   reference cl.py:16-31   initialize_cl_environment*, get_gpu_devices -> cgamd_ctx_*
 *   reference cl.py:33-42   kernels {'axpy','aypx','spmv','sub','vdot'}  -> cgamd_{axpy,aypx,spmv,sub,vdot}
 *   reference cl.py:44-200 / clcg.c:111-466   CG()/cg()                  -> cgamd_solver_* and cg()
 * plus what SURVEY §8(f) asks for: a persistent handle (matrix stays resident
 * across solves), the residual history the reference computes but drops
 * (clcg.c:274-292,384-387), status codes, and row-partitioned multi-GPU CG.
 *
 * Value types: the reference is fp32/complex64 only (clcg.h:3-5); f64/c128 are
 * added for the headline metric.  Complex values are interleaved (re,im).
 * Multiple right-hand sides are RHS-major: element i of RHS r at [i + r*size].
 *
 * All functions return CGAMD_OK (0) or a negative/positive cgamd_status; the
 * message of the last failure on the calling thread is cgamd_last_error().
 * There is no CPU fallback anywhere: without a HIP device every compute entry
 * fails with CGAMD_ERR_NO_DEVICE.
 */
#ifndef CGAMD_H
#define CGAMD_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { CGAMD_F32 = 0, CGAMD_F64 = 1, CGAMD_C64 = 2, CGAMD_C128 = 3 } cgamd_dtype;

typedef enum {
    CGAMD_OK = 0,
    CGAMD_ERR_INVALID = 1,    /* bad argument (NULL, negative size, misaligned pointer, bad dtype) */
    CGAMD_ERR_NO_DEVICE = 2,  /* no HIP device / runtime unavailable */
    CGAMD_ERR_HIP = 3,        /* a HIP runtime call failed */
    CGAMD_ERR_ALLOC = 4,
    CGAMD_ERR_IO = 5,         /* Matrix-Market file problems */
    CGAMD_ERR_COMM = 6,       /* RCCL failure / not initialised */
    CGAMD_ERR_STATE = 7       /* call order (e.g. iterate before set_rhs) */
} cgamd_status;

typedef struct cgamd_ctx cgamd_ctx;
typedef struct cgamd_solver cgamd_solver;

const char *cgamd_last_error(void);
int cgamd_version(void);
size_t cgamd_dtype_size(int dtype);

/* run-time configuration: 15 keys (INTEGRATION.md section 6 has the table).  Loop selection: "resident" (1; 0 = launched loops
 * only, 2 = cross-XCD form), "resident_min" (8), "resident_wide" (1), "resident_wide_min" (16), "resident_claim_ms" (200),
 * "two_launch" (1), "spmm_rowmajor" (1; 2 = every supported width, 0 = never).  Matrix stream: "index_codes" (1),
 * "index_codes16" (1), "index_codes_min_mb" (32), "pad_rows" (1).  Placement / cache policy: "spmv_nt", "vec_nt" (-1 = by
 * working-set size), "spmv_cycle" (64 row blocks per XCD turn), "vec_grid" (0 = auto).  A handle keeps the configuration it
 * was created under (snapshot at create); the call is thread-safe.  Unknown key: CGAMD_ERR_INVALID.  Keys that start with
 * "dev." are test / rehearsal hooks of this repository's own suite and scripts, not part of the interface. */
int cgamd_tune(const char *key, int value);

/* ---- devices / context (reference cl.py:16-31) -------------------------- */
int cgamd_device_count(void);                                /* <0 on error */
int cgamd_device_name(int device, char *buf, size_t buflen);
int cgamd_ctx_create(int device, cgamd_ctx **out);           /* owns one HIP stream + workspace */
int cgamd_ctx_destroy(cgamd_ctx *ctx);
int cgamd_ctx_set_stream(cgamd_ctx *ctx, void *stream);      /* borrow caller's stream (torch) */
void *cgamd_ctx_stream(cgamd_ctx *ctx);
int cgamd_ctx_device(cgamd_ctx *ctx);
int cgamd_ctx_synchronize(cgamd_ctx *ctx);

/* device memory helpers for hosts without torch (ctypes + numpy only) */
int cgamd_malloc(cgamd_ctx *ctx, size_t bytes, void **dptr);
int cgamd_free(cgamd_ctx *ctx, void *dptr);
int cgamd_memcpy_h2d(cgamd_ctx *ctx, void *dst, const void *src, size_t bytes);   /* synchronous */
int cgamd_memcpy_d2h(cgamd_ctx *ctx, void *dst, const void *src, size_t bytes);   /* synchronous */
int cgamd_memcpy_d2d(cgamd_ctx *ctx, void *dst, const void *src, size_t bytes);   /* async on ctx stream */
int cgamd_memset(cgamd_ctx *ctx, void *dst, int value, size_t bytes);             /* async on ctx stream */

/* ---- the five kernels of the hot path, device pointers, async on ctx stream
 * spmv : y[row + r*size] = sum_j aValues[j] * x[aCols[j] + r*size]
 *        (reference kernel/real/spmv.cl:5-50, kernel/complex/spmv.cl:7-53)
 * vdot : result[r] = sum_i a[i + r*size] * b[i + r*size]   (UNCONJUGATED,
 *        reference kernel/complex/vdot.cl:15; includes the final reduction the
 *        reference leaves to the host, clcg.c:274-279); result is a DEVICE array
 * axpy : y += a[r]*x (aSign != 0)  /  y -= a[r]*x (aSign == 0); a is a DEVICE array
 *        (reference kernel/real/axpy.cl:2-17)
 * aypx : y = a[r]*y + x            (reference kernel/real/aypx.cl:2-10)
 * sub  : result = a - b            (reference kernel/real/sub.cl:2-12)
 */
int cgamd_spmv(cgamd_ctx *ctx, int dtype, int size, long long nnz, const void *aValues,
               const int *aPointers, const int *aCols, const void *x, void *y, int nRHS);
int cgamd_vdot(cgamd_ctx *ctx, int dtype, int size, const void *a, const void *b, void *result, int nRHS);
int cgamd_axpy(cgamd_ctx *ctx, int dtype, int size, const void *x, void *y, const void *a, int aSign, int nRHS);
int cgamd_aypx(cgamd_ctx *ctx, int dtype, int size, const void *x, void *y, const void *a, int nRHS);
int cgamd_sub(cgamd_ctx *ctx, int dtype, int size, const void *a, const void *b, void *result, int nRHS);

/* ---- persistent solver handle ------------------------
 * flags for cgamd_solver_create */
#define CGAMD_MATRIX_ON_DEVICE 1   /* aValues/aPointers/aCols are device pointers, borrowed (not copied).  A borrowed value array may
                                    * be changed only between solves, and every change must be followed by cgamd_solver_refresh_values
                                    * before the next cgamd_solver_set_rhs: the handle keeps re-encodings of the values (value, joint
                                    * and row-pattern codes) and preconditioners built from them, which that call brings up to date.
                                    * aPointers / aCols must not change while the handle lives */
#define CGAMD_NO_GRAPH 2           /* plain stream launches instead of hipGraph replay */
#define CGAMD_UNFUSED 4            /* reference op structure: spmv, vdot, axpy, axpy, vdot, aypx (6 kernels) */
#define CGAMD_HERMITIAN 16         /* cgamd_solver_create / cgamd_solver_create_batched: CG for a complex HERMITIAN positive-definite
                                    * matrix -- every inner product of the recurrence conjugated, <a, b> = sum conj(a_i) b_i -- in place of
                                    * the reference's unconjugated recurrence (COCG, for complex-symmetric matrices).  See "Hermitian
                                    * systems" below cgamd_solver_hermitian.  Accepted and without effect on the real value types */
#define CGAMD_SPLIT_LONG_ROWS 1024  /* cgamd_solver_create: cut very long rows across work-groups and keep the block SpMV forms for every
                                    * other row (csrc/long_rows.hip).  Without it ONE hub row sends the whole matrix to the generic
                                    * stream kernel.  See "Long rows" below cgamd_solver_long_rows.  Accepted by every create entry and
                                    * without effect where the split does not apply */
#define CGAMD_DIST_NO_OVERLAP 32    /* cgamd_dist_create: exchange first, then one SpMV (no interior/boundary overlap) */
#define CGAMD_DIST_P2P 64            /* cgamd_dist_create: no RCCL; peers write each other's IPC mailboxes (attach_p2p) */
#define CGAMD_DIST_GRAPH 8         /* cgamd_dist_create: replay each iteration (incl. RCCL ops) from a hipGraph */
#define CGAMD_DIST_P2P_STAGED 128   /* with CGAMD_DIST_P2P: separate push / wait+unpack launches and all-reduce launches (7 per
                                     * iteration) instead of the default four-launch iteration (push and wait inside the SpMV
                                     * launch, halo read in place from the mailbox, beta all-reduce inside the aypx launch) */

#define CGAMD_DIST_SINGLE_REDUCTION 256   /* cgamd_dist_create: the single-reduction form of the recurrence (Chronopoulos-Gear: w = A r,
                                     * ONE global exchange of {r.r, w.r} per iteration instead of two, two launches per iteration with
                                     * CGAMD_DIST_P2P): the same iterates in exact arithmetic, different rounding -- opt-in, held to a
                                     * stated tolerance against the reference's iterates, not bit for bit (csrc/cg1.hip) */

#define CGAMD_DIST_RESIDENT 512      /* cgamd_dist_create: iterate() calls of at least `resident_wide_min` iterations run in ONE launch (csrc/slab.hip:
                                     * vectors in registers, matrix streamed, the two reductions as in-launch all-gathers) where the rank's
                                     * slab fits (up to ~3M rows of at most 8 entries on average, not complex128); the reference's
                                     * recurrence, results held to the oracle like the chip-wide resident loop's.  cgamd_dist_loop_launches()
                                     * reports 0 when it applies; otherwise the flag changes nothing */

int cgamd_solver_create(cgamd_ctx *ctx, int dtype, int size, long long nnz, const void *aValues,
                        const int *aPointers, const int *aCols, int nRHS, int flags, cgamd_solver **out);
/* nSystems linear systems on ONE pattern: aPointers / aCols are shared, aValues holds nSystems * nnz values, the values of
 * system r at aValues[r * nnz + j] in the order of aCols.  Right-hand side r (b, x0, x, history column r) belongs to system r;
 * the handle's nRHS is nSystems.  This is the reference's additive-Schwarz step with variable coefficients (as_prec with VarCoeff,
 * p_h-PY_C-CL.py:1970-1985: a matrix P[p] per sub-domain on the same grid), which the reference solves one sub-domain after another.
 * All four value types, any nSystems >= 1 and size >= 1; flags CGAMD_MATRIX_ON_DEVICE (the borrowed value array is nSystems * nnz
 * long; any alignment of the element type), CGAMD_NO_GRAPH, CGAMD_UNFUSED; CSR validation as in cgamd_solver_create.  aValues need
 * no padding: nnz * sizeof(value) may be any number of bytes.  cgamd_solver_reload_matrix takes nSystems * nnz new values.
 * set_rhs, iterate, get_x, history, iterations_done, solve, vector, ld, spmv (y_r = A_r x_r; fused_dot: partials of x_r . y_r),
 * dot_partials and destroy behave as on any other handle.  The handle always runs a launched loop (cgamd_solver_loop_launches() >= 2:
 * no resident, chip-wide or two-launch loop), keeps the RHS-major layout (cgamd_solver_layout() == 0) and uses no index, value or
 * joint codes (the three accessors return 0); its SpMV is family 6 of cgamd_last_spmv_form (csrc/batched.hip).
 * Not served: cgamd_solver_iterate_tol and cgamd_solver_spmm_rowmajor return CGAMD_ERR_STATE; so do the five shared-M
 * cgamd_solver_set_preconditioner* entries -- an M shared by all right-hand sides has no meaning for different systems -- except
 * cgamd_solver_set_preconditioner(s, NULL, 0), which returns CGAMD_OK and removes a per-system preconditioner if one is set.  A
 * refused call leaves the handle as it was.  Preconditioned CG runs with one M PER SYSTEM: cgamd_solver_set_preconditioner_batched,
 * _batched_jacobi and _batched_line below.
 * Byte models: every value array is counted once and the indices once, cgamd_solver_spmv_bytes = cgamd_solver_spmv_moved_bytes =
 * nnz * (nSystems * sizeof(value) + 4) + 4 * (size + 1) + 2 * size * sizeof(value) * nSystems; the iter_* entries take the same
 * matrix term. */
int cgamd_solver_create_batched(cgamd_ctx *ctx, int dtype, int size, long long nnz, const void *aValues,
                                const int *aPointers, const int *aCols, int nSystems, int flags, cgamd_solver **out);
int cgamd_solver_systems(cgamd_solver *s);   /* nSystems of a batched handle, 0 for every other handle, negative: error */
/* ---- Hermitian systems (CGAMD_HERMITIAN, csrc/hermitian.hip) ----
 * 1 when the handle runs the conjugated recurrence (created with CGAMD_HERMITIAN on CGAMD_C64 / CGAMD_C128), 0 otherwise -- also for
 * the real value types with the flag, where Hermitian is symmetric and the handle runs the loops and gives the bits it gives without
 * it; negative: error.
 * The recurrence: delta_k = r_k^H r_k (the history stores it with an imaginary part of exactly +0; it is never negative),
 * alpha = rho / Re(d^H q), beta = rho' / rho with rho = delta, both REAL and stored in the value type with imaginary part +0.  With a
 * diagonal M: z = m .* r, rho = Re(r^H z), and the history keeps r^H r.  The caller vouches for A = A^H being positive definite and
 * for m being real and positive: neither is validated (nor is the symmetry of the matrix of any other handle).
 * Such a handle runs a launched loop only: cgamd_solver_loop_launches() == 4, cgamd_solver_x_lag() == 1, cgamd_solver_layout() == 0 at
 * every nRHS; no resident, chip-wide or two-launch loop.  CGAMD_NO_GRAPH and CGAMD_MATRIX_ON_DEVICE are served;
 * CGAMD_UNFUSED | CGAMD_HERMITIAN on a complex type is CGAMD_ERR_INVALID at creation.  The SpMV forms, index, value, joint and
 * row-pattern codes included, are the ones any handle on that matrix takes.
 * Served: set_rhs (with x0), iterate, iterate_timed, get_x, history, solve, iterate_until (sqrt|delta| is the true 2-norm of r),
 * refresh_values and reload_matrix, cgamd_solver_set_preconditioner and _jacobi, on batched handles _batched and _batched_jacobi, any
 * nRHS.  Not served, CGAMD_ERR_STATE with the handle untouched: cgamd_solver_iterate_tol and the tridiagonal / line preconditioner
 * entries (_tridiag, _tridiag_strided, _line, _batched_line); cgamd_solver_step_plan / _step_state: CGAMD_ERR_INVALID.
 * cgamd_solver_spmv(..., fused_dot) stays the development entry it is (unconjugated x.y).  cgamd_dist_create refuses the flag
 * (CGAMD_ERR_INVALID).  Byte models: cgamd_solver_iter_bytes and cgamd_solver_iter_moved_bytes count 12 vector passes, 14 with a
 * diagonal M: the launched loop's 10 / 12 and conj(d), written by the d step and read by the SpMV's fused dot. */
int cgamd_solver_hermitian(cgamd_solver *s);
/* development accessor (tests): alpha and beta of the last iteration, nRHS values of the handle's type each, copied to the host
 * after the handle's stream has drained; either pointer may be NULL.  CGAMD_HERMITIAN handles only (CGAMD_ERR_STATE otherwise: the
 * other handles have cgamd_solver_step_state) */
int cgamd_solver_hermitian_scalars(cgamd_solver *s, void *alpha_host, void *beta_host);
int cgamd_solver_destroy(cgamd_solver *s);
/* new values / pattern of the SAME size (size, nnz, nRHS, dtype) into a handle that owns its matrix (created from host
 * arrays): keeps allocations, stream and -- when the row pointers are unchanged -- the plan and the captured graphs.
 * The next call must be cgamd_solver_set_rhs.  A preconditioner from the caller's arrays is kept; one built from the matrix
 * (cgamd_solver_set_preconditioner_line / _jacobi; on a batched handle _batched_line / _batched_jacobi / _batched_multigrid) is built
 * again from the new matrix. */
int cgamd_solver_reload_matrix(cgamd_solver *s, const void *aValues, const int *aPointers, const int *aCols);
/* New VALUES on the SAME pattern.  Everything the handle made from the values follows them (the value, joint and row-pattern codes
 * of the SpMV, a preconditioner built from the matrix); nothing made from the pattern alone is touched: no CSR validation, no plan,
 * no resident-plan scan, no change of the x lag, the column codes stay.
 *   a handle that BORROWS its matrix (CGAMD_MATRIX_ON_DEVICE): aValues is NULL, or the borrowed pointer itself with on_device = 1 --
 *     "the array I lent you has changed in place".  Any other pointer: CGAMD_ERR_INVALID, handle untouched (copy the new values into
 *     the borrowed array; another array needs a new handle, pointer alignment decides kernel forms).
 *   a handle that OWNS its matrix: aValues holds nnz values (a batched handle: nSystems * nnz), host (on_device = 0) or device
 *     (on_device = 1, copied on the handle's stream) memory.  NULL: CGAMD_ERR_INVALID.
 * The call waits for the handle's stream before it reads the values; a caller who wrote the borrowed array on ANOTHER stream orders
 * that write before this call (synchronise that stream, or make the handle's stream wait for it).  The next call must be
 * cgamd_solver_set_rhs (cgamd_solver_iterate returns CGAMD_ERR_STATE until then).  Inside a stream capture: CGAMD_ERR_INVALID.
 * Codes: where every class of equal values of the old matrix still holds one value (a constant-coefficient operator with rescaled
 * coefficients) one pass over the values finds that out and only the dictionaries are rewritten, in place: no code array, no pointer
 * and no captured graph changes.  cgamd_solver_value_codes / _joint_codes / _row_codes then keep reporting the dictionary entries in
 * use, which may exceed the number of distinct values / pairs / patterns when classes have merged.  Otherwise the three codes are
 * freed and built again as at creation (the graphs are captured again); values that no longer qualify (more than 256 of them, or
 * the all-ones NaN pattern) run the form that reads aValues, and a handle that had no value codes gains them when the new values
 * qualify.  Results are, bit for bit, those of a fresh handle created from the new values.
 * Preconditioners: one from the caller's arrays is kept; one built from the matrix (cgamd_solver_set_preconditioner_jacobi / _line,
 * _batched_jacobi / _batched_line / _batched_multigrid) is built again from the new values, same kind, stride and arguments.  If that fails the values are in force,
 * the preconditioner is removed and the error naming the row (batched: the system and the row) is returned. */
int cgamd_solver_refresh_values(cgamd_solver *s, const void *aValues, int on_device);
/* what the last cgamd_solver_refresh_values did: 0 no refresh yet, or the handle carries no codes of its values (multi-RHS, batched,
 * complex128, below the size thresholds, handles of the resident loops that build none); 1 dictionaries rewritten, arrays and graphs
 * kept; 2 value, joint and row codes built again; 3 the new values do not qualify, the SpMV reads aValues; negative: error */
int cgamd_solver_last_refresh(cgamd_solver *s);
/* iteration graphs this handle has captured since it was created (0 with CGAMD_NO_GRAPH).  A handle replays the graphs it has; the
 * count grows only when something invalidated them -- so it does not grow across a refresh that kept them (outcome 1). */
int cgamd_solver_graph_captures(cgamd_solver *s);
/* b, x0: nRHS*size values, host (on_device=0) or device (on_device=1) memory; x0 may be NULL (zeros).
 * Computes r = b - A x0, d = r, delta0 = r.r  (reference clcg.c:255-292) and resets the iteration count. */
int cgamd_solver_set_rhs(cgamd_solver *s, const void *b, const void *x0, int on_device);
/* Run exactly nIterations iterations (reference clcg.c:297-419).  Handles on a LAUNCHED loop (cgamd_solver_loop_launches() >= 2)
 * only enqueue: asynchronous, no host sync.  Handles on a RESIDENT loop (loop_launches() 0 or 1, calls of at least
 * "resident_min" / "resident_wide_min" iterations) synchronise: the call takes the GPU's resident-launch lock (one resident
 * grid per GPU at a time, across processes; at most "resident_claim_ms" of waiting), launches, and waits for the kernel before
 * it releases the lock -- so it returns with the iterations done.  When the lock or the CUs cannot be had in that time the call
 * runs the same iterations on the handle's launched loop instead (asynchronous again); results are those of that loop. */
int cgamd_solver_iterate(cgamd_solver *s, int nIterations);
/* Tolerance stop on the device (one right-hand side; handles whose loop is resident, cgamd_solver_loop_launches() < 2): runs until
 * sqrt|r.r| < tol (or NaN), at most maxIterations; *iterations_run = iterations of this call; x is the iterate of exactly that
 * many (reference: the `tol` loop of p_h-PY_C-CL.py:1338-1369).  CGAMD_ERR_STATE if the handle runs a launched loop. */
int cgamd_solver_iterate_tol(cgamd_solver *s, int maxIterations, double tol, int *iterations_run);
/* Tolerance stop PER RIGHT-HAND SIDE on the device, for the LAUNCHED loops: the reference's sub-domain loop
 * `r[p] = CG(P[0], z[p].ravel(), tol=CGtol, maxit=CGMaxIT)` (p_h-PY_C-CL.py:1916-1921, the `tol` loop at 1338-1369; PCG:
 * helmFE_var.py:580-584) as one batched solve.  Right-hand side r stops in the first iteration k >= 1 of such a call for which
 * !(sqrt|delta_k[r]| >= tol_r), delta_k = r_k . r_k (unconjugated) being the value the history records -- with a preconditioner
 * still r.r, not rho; NaN stops; the test is evaluated in double.  tol: nTol = 1 (one for all) or nRHS positive values, host
 * memory.  A stopped right-hand side is FROZEN: cgamd_solver_get_x returns for its column the iterate of exactly its stopping
 * iteration -- the bits of set_rhs; iterate(its_r) on this handle -- while the others run on until each has stopped or
 * maxIterations iterations of this call are done.  iterations_run[r] (nRHS ints): iterations of right-hand side r since set_rhs,
 * its stopping iteration or the handle's count; cgamd_solver_iterations_done is their maximum.  History rows k <= its_r of column r
 * are those of a fixed-count run, rows its_r < k <= iterations_done repeat delta_{its_r}.  maxIterations == 0 returns the current
 * counts at once.
 * The call synchronises, but never per iteration: it enqueues chunks of checkEvery iterations (0 = 8), reads one device word -- the
 * number of active right-hand sides -- asynchronously after each, and waits for the word of chunk c - 1 once chunk c is enqueued.
 * Iterations enqueued after the last stop change nothing, so the result does not depend on checkEvery.  The call may follow
 * cgamd_solver_iterate calls (their iterations are not examined again) and may be repeated: until(a); until(b) leaves the bits of
 * until(a + b); a stopped right-hand side stays stopped until the next cgamd_solver_set_rhs, whatever the later tolerances.  Once
 * a right-hand side has stopped, cgamd_solver_iterate, _iterate_timed and _iterate_tol return CGAMD_ERR_STATE until
 * cgamd_solver_set_rhs (the columns are at different iterations).
 * Served: every handle whose vectors are RHS-major (cgamd_solver_layout() == 0) -- all value types, any nRHS, diagonal and
 * tridiagonal (stride 1 short and long form, stride > 1) preconditioners, batched handles with and without a per-system
 * preconditioner, CGAMD_NO_GRAPH, CGAMD_MATRIX_ON_DEVICE.  The call runs the handle's three / four-launch loop (six with the long
 * sweep); a handle whose cgamd_solver_iterate takes a resident or the two-launch loop runs that launched loop from this call to the
 * next cgamd_solver_set_rhs, with the same bits (cgamd_solver_iterate_tol then returns CGAMD_ERR_STATE).
 * CGAMD_ERR_INVALID: NULL s / tol / iterations_run, nTol not in {1, nRHS}, a tolerance that is not > 0, negative maxIterations or
 * checkEvery.  CGAMD_ERR_STATE, the handle untouched: row-major layout (cgamd_solver_layout() == 1), CGAMD_UNFUSED, no set_rhs. */
int cgamd_solver_iterate_until(cgamd_solver *s, int maxIterations, const double *tol, int nTol, int checkEvery, int *iterations_run);
/* Residual replacement with the search direction kept (van der Vorst and Ye, "reliable updates"): hands a running handle a new
 * residual without resetting its direction, so that a caller who keeps x and the true residual elsewhere -- in a wider type, see
 * cgamd_mixed_solve -- goes on in the SAME Krylov space.  r_new: a DEVICE pointer to nRHS * size values of the handle's type at stride
 * `size`.  Enqueued on the handle's stream (no host synchronisation).  It sets r := r_new (padding rows 0), x := 0, delta := r.r and,
 * with a diagonal M, z = m .* r and rho := r.z; d STAYS AS IT IS.  The iteration counter is 0 again, the history restarts with row 0 =
 * r.r, the stop record of cgamd_solver_iterate_until is disarmed and every right-hand side is active again.  The sums are taken by the
 * launches, and in the order, by which cgamd_solver_set_rhs takes delta0 and rho0: history row 0 and delta are the bits a fresh
 * handle shows after set_rhs(b = r_new, x0 = NULL).  cgamd_solver_iterate and _iterate_until then continue the recurrence from
 * (0, r_new, d): the first beta is rho_1 / rho_0 of the NEW residual.
 * From this call to the next cgamd_solver_set_rhs the handle runs the launched loop cgamd_solver_iterate_until runs, d in one buffer
 * and final in memory.  A handle that has just iterated on its two-launch or a resident loop holds the direction of its last
 * iteration and leaves d = beta d + r to the next SpMV launch: the call completes that step first (with the OLD residual, which is
 * part of the direction that is kept), exactly as cgamd_solver_iterate_until does, and cgamd_solver_vector(s, 2) then names that buffer.
 * Served: RHS-major handles (cgamd_solver_layout() == 0), all four value types, any nRHS, no preconditioner or a diagonal one,
 * CGAMD_NO_GRAPH, CGAMD_MATRIX_ON_DEVICE.  CGAMD_ERR_STATE, the handle untouched: no cgamd_solver_set_rhs yet, row-major layout, a
 * tridiagonal / line preconditioner, CGAMD_HERMITIAN on a complex type, batched handles, CGAMD_UNFUSED.  CGAMD_ERR_INVALID: NULL
 * arguments, or a call while the handle's stream is being captured. */
int cgamd_solver_replace_residual(cgamd_solver *s, const void *r_new);
/* nIterations iterations with plain launches and a HIP event pair around every SpMV launch on the solver's stream;
 * returns the average in-loop SpMV duration (and optionally the average iteration time), in ms.  Synchronises. */
int cgamd_solver_iterate_timed(cgamd_solver *s, int nIterations, float *spmv_ms_avg, float *iter_ms_avg);
/* copy the current iterate; synchronises the stream when on_device == 0 */
int cgamd_solver_get_x(cgamd_solver *s, void *x, int on_device);
/* residual history: entry k (k = 0..iterations done) holds delta_k[r] for r < nRHS, value type = dtype.
 * Synchronises.  Returns the number of entries written (<= max_entries) or a negative status. */
int cgamd_solver_history(cgamd_solver *s, void *history, int max_entries);
int cgamd_solver_iterations_done(cgamd_solver *s);
/* device pointers of the solver's resident state (for zero-copy inspection): which = 0:x 1:r 2:d 3:q */
void *cgamd_solver_vector(cgamd_solver *s, int which);
/* leading dimension (values between consecutive right-hand sides) of the handle's own vectors: `size` rounded up to a whole number
 * of 16-byte packs (2 values in fp64 / complex64, 4 in fp32) -- the handle carries such systems with 1-3 empty rows appended so that
 * every right-hand side stays 16-byte aligned; b / x0 / x in the caller's arrays keep stride `size` (tuning key "pad_rows" 0: as passed) */
int cgamd_solver_ld(cgamd_solver *s);
/* Diagonal (Jacobi) preconditioning -- the reference's PCG(A, b, M) with a diagonal CSR M, z = M.dot(r)
 * (helmFE_var.py:546-586).  m: `size` values of the solver's type (1/diag(A) for Jacobi), host or
 * device; NULL removes it.  Takes effect at the next cgamd_solver_set_rhs; history keeps holding r.r (the stopping
 * test of the reference, helmFE_var.py:580-584), the recurrence uses rho = r.z.  Handles the chip-wide resident loop can take over
 * (cgamd_solver_loop_launches() == 1 once the preconditioner is set) run the recurrence inside that loop, with the bits of the
 * four-launch PCG loop of the same handle; cgamd_solver_iterate_tol then stops it on the device. */
int cgamd_solver_set_preconditioner(cgamd_solver *s, const void *m, int on_device);
/* Tridiagonal M: the reference PCG's spsolve branch (helmFE_var.py:561-562): z solves M z = r.
 * lower[i] = M[i][i-1] (lower[0] ignored), diag[i] = M[i][i], upper[i] = M[i][i+1] (upper[size-1] ignored):
 * `size` values each, the solver's value type, host (on_device = 0) or device memory.  M is shared by all right-hand sides, every
 * value type.  Factored once here (Thomas LU in double / complex double, NO pivoting); CGAMD_ERR_INVALID, with the row in
 * cgamd_last_error, on a non-finite entry or a zero / non-finite pivot -- the handle is then unchanged.  Like the diagonal form it
 * takes effect at the next cgamd_solver_set_rhs, history keeps holding r.r and rho = r.z drives alpha and beta; it replaces a
 * diagonal preconditioner, cgamd_solver_set_preconditioner replaces it, and cgamd_solver_set_preconditioner(s, NULL, 0) removes
 * either (the handle then returns the bits of one that never had a preconditioner).  cgamd_solver_reload_matrix keeps it.
 * Launched loop only: no resident loop takes the recurrence (cgamd_solver_loop_launches() = 4, or 6 when a coupled line is longer
 * than one work-group's chunk -- 2048 rows f32, 1024 f64 / complex64, 512 complex128 -- and the sweep takes three launches);
 * cgamd_solver_iterate_tol returns CGAMD_ERR_STATE (check the history from the host).  Padding rows (cgamd_solver_ld) are
 * decoupled, z = 0 there. */
int cgamd_solver_set_preconditioner_tridiag(cgamd_solver *s, const void *lower, const void *diag, const void *upper, int on_device);
/* The same M along any grid axis: a line preconditioner whose coupled rows lie `stride` apart (stride = nx for the y-lines,
 * nx * ny for the z-lines of a grid numbered x fastest), so that strong coupling off the fastest index needs no permutation of the
 * matrix (which would give up the one-byte codes of the SpMV).  lower[i] = M[i][i-stride] (ignored for i < stride), diag[i] =
 * M[i][i], upper[i] = M[i][i+stride] (ignored for i >= size - stride): `size` values each, the solver's value type, host or device
 * memory, every value type, M shared by all right-hand sides.  stride == 1 IS cgamd_solver_set_preconditioner_tridiag (same code
 * path, same bits); stride < 1 or stride >= size returns CGAMD_ERR_INVALID.  In every other respect the contract of the stride-1
 * form: factored once here (Thomas LU in double / complex double, NO pivoting) along every chain c, c + stride, c + 2 stride, ...;
 * CGAMD_ERR_INVALID with the row in cgamd_last_error on a non-finite entry or a zero / non-finite pivot, the handle then unchanged;
 * effective at the next cgamd_solver_set_rhs; history keeps r.r, rho = r.z drives alpha and beta; it replaces a diagonal or
 * stride-1 preconditioner and either of those replaces it, cgamd_solver_set_preconditioner(s, NULL, 0) removes it (the handle then
 * returns the bits of one that never had a preconditioner); cgamd_solver_reload_matrix keeps it; padding rows are decoupled, z = 0
 * there; launched loop only, cgamd_solver_loop_launches() = 4, cgamd_solver_iterate_tol returns CGAMD_ERR_STATE.
 * A chain is cut into segments where both stored couplings round to zero in the value type -- on a grid the segments are the grid
 * lines, nx * nz y-lines of ny rows or nx * ny z-lines of nz rows -- and the device solves ONE SEGMENT PER THREAD, consecutive
 * segments in consecutive threads: with thousands of lines whose first rows are consecutive every step of the sweep moves whole
 * cache lines.  A segment may have any length, but a matrix with FEW LONG segments (a 1-D chain at stride 2: two segments) is solved
 * correctly and serially within each segment, i.e. slowly; the form is meant for grids. */
int cgamd_solver_set_preconditioner_tridiag_strided(cgamd_solver *s, int stride, const void *lower, const void *diag,
                                                    const void *upper, int on_device);
/* The line preconditioner of the handle's OWN matrix: M = the entries of A at column - row in {-stride, 0, +stride} (stride 1: the
 * x-lines; nx: the y-lines; nx * ny: the z-lines of a grid numbered x fastest), extracted, factored and planned ON THE DEVICE -- a
 * few passes over the matrix instead of three arrays cut out on the host and a serial factorisation there.  Everything not said here
 * is the contract of cgamd_solver_set_preconditioner_tridiag_strided: same recurrence (l = a / u_prev, u = b - l c_prev, w = 1 / u
 * in double / complex double, -l, -w c and w rounded once to the value type), same factor layout, same segment rule, same plan, same
 * sweep kernels (stride 1: the scan sweep, 4 or 6 launches per iteration; stride > 1: one thread per segment), same errors with the
 * same wording -- the row named is the smallest failing one -- and nothing on the handle changes on failure (a preconditioner set
 * before stays in force).  Factors may differ from the array entries' in the last place (the host divides through complex
 * arithmetic); results are held to tolerances against them and are bit-stable from call to call.
 * Every handle: one that owns its matrix or borrows it (CGAMD_MATRIX_ON_DEVICE: the values as they are at the time of the call),
 * every value type, any nRHS, whatever codes the SpMV runs on.  stride < 1 or stride >= size returns CGAMD_ERR_INVALID.
 * Extraction: the columns of a row may be unsorted; entries of a row at the same column are summed in stored order in double /
 * complex double, as the SpMV adds them up; a row without a stored diagonal has diagonal 0 (a zero pivot); padding rows stay
 * decoupled.  Temporary device memory: three `size`-long value arrays and O(size) bytes of flags, freed before return; no array of
 * `size` values crosses to the host.
 * The factorisation runs one thread per pre-segment (a chain cut where both couplings of A are exactly zero; the final segments
 * refine these).  LONG SEGMENTS: when the longest pre-segment exceeds 65536 rows (a 1-D chain; a provisional limit: the table of
 * scripts/line_setup_ab.py that is to set it, device against host per segment length, is not measured yet) the diagonals are extracted on the device and
 * then take the host route of the array entry -- same contract, slower setup, source 3 below.
 * cgamd_solver_reload_matrix REBUILDS a preconditioner made by this entry or by cgamd_solver_set_preconditioner_jacobi from the new
 * matrix (same kind, same stride); if that fails the matrix is loaded, the preconditioner is removed and the call returns the error
 * naming the row.  Preconditioners from the caller's arrays are kept as they are. */
int cgamd_solver_set_preconditioner_line(cgamd_solver *s, int stride);
/* Jacobi from the handle's own matrix: m[i] = 1 / A[i][i] built on the device (entries at the same column summed as above, the
 * division in double / complex double, rounded once to the value type), then exactly cgamd_solver_set_preconditioner's diagonal
 * form, resident loops included.  A zero, missing or non-finite diagonal returns CGAMD_ERR_INVALID naming the first such row, the
 * handle unchanged. */
int cgamd_solver_set_preconditioner_jacobi(cgamd_solver *s);
/* Preconditioned CG on a BATCHED handle (cgamd_solver_create_batched): one M per system, M_r for right-hand side r.  The three entries
 * (and cgamd_solver_set_preconditioner_batched_multigrid below) are for batched handles only; on any other handle they return
 * CGAMD_ERR_STATE naming the shared-M entry to use instead.
 * Everything not said here is the contract of the one-matrix entries above: effective at the next cgamd_solver_set_rhs; history keeps
 * holding r.r; rho = r.z drives alpha and beta per system; cgamd_solver_set_preconditioner_batched(s, NULL, 0) or
 * cgamd_solver_set_preconditioner(s, NULL, 0) removes it and the handle then returns the bits of one that never had a
 * preconditioner; a failed call leaves the handle as it was (a preconditioner set before stays in force with the same bits);
 * cgamd_solver_iterate_tol keeps returning CGAMD_ERR_STATE; CGAMD_NO_GRAPH, CGAMD_UNFUSED (the preconditioned loop is the same four
 * launches, d.q partials included) and CGAMD_MATRIX_ON_DEVICE (the values as they are at the time of the call) are served.
 *   _batched         m: nSystems * size values of the handle's type, host or device, the diagonal of system r at m + r * size (the
 *                    caller's stride is `size`; inside the handle it is cgamd_solver_ld and the padding rows are 0); z_r = m_r .* r_r.
 *                    m == NULL removes any preconditioner.  Source 1; kept by cgamd_solver_reload_matrix.
 *   _batched_jacobi  m_r[i] = 1 / A_r[i][i] from every system's values, by the rules of cgamd_solver_set_preconditioner_jacobi (entries
 *                    at the same column summed in stored order in double / complex double, one rounding).  Source 2.
 *   _batched_line    M_r = the entries of A_r at column - row in {-stride, 0, +stride}; stride outside [1, size - 1] returns
 *                    CGAMD_ERR_INVALID.  Every system is factored with the recurrence of cgamd_solver_set_preconditioner_line (Thomas, no
 *                    pivoting, double / complex double; -l, -w c and w each rounded once).  Source 2.
 * Errors (CGAMD_ERR_INVALID) name the system and the row, "... in system R row I": the smallest failing system, then the smallest row in
 * it; the wording is otherwise that of the one-matrix entries (zero, missing or non-finite diagonal; non-finite entry; zero or
 * non-finite pivot; pivot too small).
 * ONE SEGMENT PLAN serves all systems: row i starts a segment when i < stride or when, in EVERY system, both stored couplings to row
 * i - stride round to zero in the value type (the one-matrix rule AND-ed over the systems; on a grid the segments are the grid
 * lines).  A system with a further zero coupling inside a shared segment is solved correctly: its zero factors restart the
 * recurrence arithmetically.  stride 1 takes the scan sweep on chunks built from the shared starts (cgamd_solver_loop_launches() = 4,
 * or 6 when a shared segment is longer than a chunk), stride > 1 one thread per segment (4 launches).
 * The setup runs on the device with a constant number of launches and host synchronisations whatever nSystems (extraction reads the
 * pattern once per row and then the found positions in every system's values; one thread per (pre-segment, system) factors).  There is
 * no host route and no row limit: source 3 does not occur, and LONG 1-D CHAINS ARE FACTORED AND SOLVED SERIALLY, one thread per
 * (segment, system) in the setup -- correct, and slow.  Temporary device memory: six nSystems * size value arrays.
 * cgamd_solver_reload_matrix rebuilds the Jacobi or line form from the nSystems * nnz new values; if that fails the matrices are
 * loaded, the preconditioner is removed and the error is returned.
 * Byte models (on top of the matrix term nnz * (nSystems * V + 4) + 4 * (size + 1), V = sizeof(value); moved and algorithmic alike):
 * diagonal 12 * size * V * nSystems; line at stride > 1 (14 + 3); at stride 1 (11 + 3), in its long form (13 + 6) -- the vector passes
 * of the one-matrix forms and the three factor arrays, now read per system. */
int cgamd_solver_set_preconditioner_batched(cgamd_solver *s, const void *m, int on_device);
int cgamd_solver_set_preconditioner_batched_jacobi(cgamd_solver *s);
int cgamd_solver_set_preconditioner_batched_line(cgamd_solver *s, int stride);
/* ---- Aggregation multigrid for grid systems (csrc/multigrid.hip, csrc/multigrid_setup.cpp) ----
 * z = M^-1 r is one V-cycle on a hierarchy built ON THE DEVICE from the handle's own matrix: the preconditioner that cuts the
 * NUMBER of iterations of an isotropic stencil system, where Jacobi does nothing and the lines pay off only under anisotropy.
 * The rows are the nodes of an nx x ny x nz grid numbered x fastest (nx * ny * nz == size; nz = 1 or ny = nz = 1: 2-D, 1-D).
 *   Aggregates: fine node (x, y, z) -> coarse node (x >> 1, y >> 1, z >> 1) of the ceil(nx / 2) x ceil(ny / 2) x ceil(nz / 2) grid, x
 *     fastest; an axis of length 1 stays 1; odd lengths leave aggregates of 1, 2 or 4 nodes at the far faces.  Coarsening repeats
 *     while a level has more than min_rows rows, at most 16 levels.  Padding rows (cgamd_solver_ld) belong to no aggregate, z = 0 there.
 *   Coarse matrices: A_c = P^T A P with piecewise-constant P -- entry (I, J) is the sum of the fine entries (i, j) with agg(i) = I,
 *     agg(j) = J, fine rows ascending and entries in stored order, in double / complex double, rounded once.  Columns ascending,
 *     structural zeros kept.  A coarse row with more than 64 distinct columns: CGAMD_ERR_INVALID naming the level and the row.
 *   Per level: dinv = 1 / diag by the rules and with the error wording of cgamd_solver_set_preconditioner_jacobi (the level is named
 *     too), and lmax = max_i |dinv_i| sum_j |a_ij| in double, the Gershgorin bound of D^-1 A.
 *   Smoother S_s(b, x) on [lmax / kappa, lmax], theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta, rho_0 =
 *     1 / sigma: first step d = (1 / theta) (dinv (b - A x)) (x = 0: dinv b, no product), x += d; step k >= 1: rho_k = 1 / (2 sigma -
 *     rho_{k-1}), d = (rho_k rho_{k-1}) d + (2 rho_k / delta) (dinv (b - A x)), x += d.  The coefficients are computed on the host in
 *     double and passed rounded to the real type.  kappa = 4 and smooth_steps steps on every level but the coarsest, which takes
 *     kappa = 30 and 8 steps from x = 0.
 *   V(l): x = S(b, 0); b_{l+1}[I] = sum over i in I, ascending, of (b - A x)[i]; e = V(l + 1); x[i] += over_correction e[agg(i)];
 *     x = S(b, x).
 * Every sum has a fixed order: the same bits from run to run and however a solve is cut into calls.  The cycle is a linear chain of
 * launches inside the handle's captured iteration graphs (CGAMD_NO_GRAPH: plain launches, same bits).
 * smooth_steps 0 ... 4 (0 = 1), over_correction finite and >= 0 (0 = 1.6), min_rows >= 0 (0 = 512).  Takes effect at the next
 * cgamd_solver_set_rhs; history keeps r.r, rho = r.z drives alpha and beta; replaces any other preconditioner and is replaced by any
 * other; cgamd_solver_set_preconditioner(s, NULL, 0) removes it and the handle then returns the bits of one that never had it.  On
 * failure the handle is unchanged.  cgamd_solver_preconditioner_source() reports 2.  cgamd_solver_refresh_values and
 * cgamd_solver_reload_matrix build the hierarchy again from the new values; if that fails the preconditioner is removed and the error
 * returned.  Launched loop only: per iteration SpMV, cg_alpha, r update, the V-cycle, r.z, update -- cgamd_solver_loop_launches() = 5 +
 * the cycle's launches (5 per level above the coarsest, 1 on level 0, 14 on the coarsest, with one smoothing step).
 * Served: all four value types, any nRHS (RHS-major), CGAMD_MATRIX_ON_DEVICE, CGAMD_NO_GRAPH, cgamd_solver_iterate_until (the V-cycle
 * runs unguarded: z of a frozen right-hand side is read by nothing that writes).  CGAMD_ERR_INVALID: nx * ny * nz != size, a
 * dimension < 1, smooth_steps outside 0 ... 4, over_correction not finite or negative, min_rows negative.  CGAMD_ERR_STATE, the handle
 * untouched: batched handles, CGAMD_HERMITIAN on a complex type, handles that keep their block row-major, CGAMD_UNFUSED; with the
 * preconditioner set, cgamd_solver_iterate_tol and cgamd_solver_replace_residual (and so cgamd_mixed_solve).
 * Byte models (cgamd_solver_iter_bytes / _iter_moved_bytes), V = sizeof(value): matrix + 12 size V nRHS + m_0 SpMV_0 + sum over the
 * coarse levels l of m_l (nnz_l (V + 4) + 4 (n_l + 1) + 2 n_l V nRHS) + the vector passes of the cycle's own kernels; m_l = SpMVs
 * of a cycle on level l (2 smooth_steps; 7 on the coarsest), SpMV_0 = cgamd_solver_spmv_bytes / _spmv_moved_bytes of this handle. */
int cgamd_solver_set_preconditioner_multigrid(cgamd_solver *s, int nx, int ny, int nz, int smooth_steps, double over_correction, int min_rows);
/* levels of the hierarchy in force (0: no multigrid preconditioner; negative: error) */
int cgamd_solver_mg_levels(cgamd_solver *s);
/* info: rows, non-zeros, nx, ny, nz of the level and, in info[5], the bits of the double lmax */
int cgamd_solver_mg_level(cgamd_solver *s, int level, long long info[6]);
/* Development entries (tests; same standing as cgamd_solver_step_state).  _mg_level_matrix: the CSR arrays of a level to the host
 * (rows + 1 ints, nnz ints, nnz values; any pointer may be NULL); synchronises.  _mg_apply: z = one V-cycle of r on caller vectors,
 * device pointers to nRHS * size values at stride `size`; synchronises. */
int cgamd_solver_mg_level_matrix(cgamd_solver *s, int level, int *ptr, int *cols, void *vals);
int cgamd_solver_mg_apply(cgamd_solver *s, const void *r_dev, void *z_dev);
/* ---- Aggregation multigrid on a BATCHED handle (csrc/multigrid_batched.hip, csrc/multigrid_setup.cpp) ----
 * One hierarchy PER SYSTEM on a batched handle (cgamd_solver_create_batched): for right-hand side r, z_r is one V-cycle of r_r on the
 * hierarchy that cgamd_solver_set_preconditioner_multigrid builds on a single-system handle made from A_r with the same arguments.
 * For batched handles only: any other handle gets CGAMD_ERR_STATE naming cgamd_solver_set_preconditioner_multigrid (which, like
 * cgamd_solver_set_preconditioner_amg, keeps refusing batched handles; there is no batched algebraic form: aggregates matched from
 * the values would give every system a pattern of its own).  Everything not said here is the contract of the single-system entry,
 * restated per system: aggregates, Galerkin sums and their order, dinv, lmax, the smoother, V(l), the defaults (0 = 1 step, 1.6, 512),
 * the 16 levels, padding rows, the argument rules (CGAMD_ERR_INVALID).
 *   Shared by the systems: the box aggregates; ptr / cols of every level (the coarse pattern comes from the pattern alone, structural
 *     zeros kept, so it is the pattern every single-system handle would get); the level vectors, nSystems wide; over_correction.
 *   Per system: the coarse values, nSystems * nnz_l per level, system r at r * nnz_l (the layout of aValues); dinv, system r at r * ld
 *     of the level; lmax_r, hence the Chebyshev coefficients of every level -- computed on the host in double from each lmax_r, rounded
 *     to the real type and kept in a small device array indexed by (step, system).
 * The setup takes a constant number of launches and host synchronisations per level whatever nSystems is; the host reads the coarse
 * non-zero count, the error words and nSystems bound words.  The coarse values and bounds have the BITS of the single-system handles'
 * (the sums have a stated order).  Whether z_r has the bits of the single-system cycle depends on the summation order of the batched
 * SpMV against the single-system one, which nothing promises.
 * Takes effect at the next cgamd_solver_set_rhs; history keeps r.r, rho = r.z per system.  Replaces and is replaced by the other
 * per-system preconditioners; cgamd_solver_set_preconditioner_batched(s, NULL, 0) or cgamd_solver_set_preconditioner(s, NULL, 0)
 * removes it and the handle then returns the bits of one that never had it.  On failure the handle is unchanged and a preconditioner
 * set before stays in force with the same bits.  cgamd_solver_preconditioner_source() reports 2.  cgamd_solver_refresh_values and
 * cgamd_solver_reload_matrix build all hierarchies again from the nSystems * nnz new values; if that fails the preconditioner is
 * removed and the error returned.
 * Served: all four value types, any nSystems >= 1, CGAMD_MATRIX_ON_DEVICE, CGAMD_NO_GRAPH, cgamd_solver_iterate_until (the cycle runs
 * unguarded, as on the single handle).  CGAMD_ERR_STATE, the handle untouched: CGAMD_HERMITIAN on a complex type, CGAMD_UNFUSED.
 * cgamd_solver_iterate_tol and cgamd_solver_replace_residual keep refusing batched handles.
 * Errors about diagonals and bounds name "system R level L row I" (bounds: system and level): the smallest failing system, then the
 * smallest row.  The 64-column error names the level and the row: a property of the pattern, the same for all systems.
 * Loop: SpMV (batched), cg_alpha, r update, the cycle, r.z, update -- cgamd_solver_loop_launches() = 5 + the cycle's launches by the
 * single entry's formula: the launch count of ONE system whatever nSystems is.
 * Byte models (cgamd_solver_iter_bytes / _iter_moved_bytes), V = sizeof(value): the single entry's model with every value array and
 * dinv counted per system -- matrix nnz (nSystems V + 4) + 4 (size + 1), + 12 size V nSystems + m_0 SpMV_0 + sum over the coarse levels
 * l of m_l (nnz_l (nSystems V + 4) + 4 (n_l + 1) + 2 n_l V nSystems) + the vector passes of the cycle's kernels, each pass nSystems wide
 * and every dinv read nSystems n_l V.
 * cgamd_solver_mg_levels, _mg_level (info[5] = the bits of the LARGEST lmax_r), _mg_aggregates and _mg_apply serve the batched
 * hierarchy; _mg_level_matrix hands out nSystems * nnz_l values, system-major.
 * cgamd_solver_mg_level_bounds (a development entry like _mg_level_matrix): lmax_r of the level for r < count, count <= nSystems; it
 * also serves single-system handles (count <= 1). */
int cgamd_solver_set_preconditioner_batched_multigrid(cgamd_solver *s, int nx, int ny, int nz, int smooth_steps, double over_correction, int min_rows);
int cgamd_solver_mg_level_bounds(cgamd_solver *s, int level, double *lmax, int count);
/* ---- Algebraic aggregation multigrid (csrc/amg.hip, csrc/multigrid_setup.cpp) ----
 * The same V-cycle on a hierarchy whose aggregates are chosen FROM THE MATRIX, on the device: for a matrix that comes without a grid
 * (a Matrix-Market file, a permuted or reordered grid matrix, a mesh or graph Laplacian) and for anisotropic or variable coefficients,
 * where boxes coarsen across weak couplings.  Everything not said here is the contract of cgamd_solver_set_preconditioner_multigrid:
 * the Galerkin sums, dinv and lmax, the smoother, V(l), when it takes effect, what it replaces and what removes it, the failure rule,
 * cgamd_solver_preconditioner_source() reports 2, refresh_values / reload_matrix (the hierarchy is built again from the new values,
 * aggregates included: the bits of a fresh handle), the handles served and refused, cgamd_solver_iterate_tol and
 * cgamd_solver_replace_residual refused with it set, the launch count, the byte models (the cycle's vector passes now include the map
 * reads: 32 bytes per coarse row in the restriction, 4 per fine row in the prolongation) and the 16 levels.
 *   One PASS of deterministic handshake matching on a matrix B (n rows), strength threshold theta:
 *     strength  s_ij = -Re(b_ij) in double for every stored entry with j != i (a column stored twice is judged entry by entry);
 *       smax_i = the largest s_ij of row i that is > 0, else 0; entry (i, j) is strong when s_ij > 0 and s_ij >= theta * smax_i
 *       (the product in double; a NaN is never strong).
 *     rounds, at most 32, two launches each.  pick: every unmatched row i takes, among its strong entries whose column j was
 *       unmatched when the round began, the one with the larger s_ij, then the larger h(i, j), then the smaller j: pick[i] = j, or -1.
 *       handshake: i and j are matched when pick[i] == j and pick[j] == i.  h(i, j) in 32-bit unsigned arithmetic: lo = min(i, j),
 *       hi = max(i, j), h = (lo * 0x9E3779B1) ^ hi; h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *       (not the index: by index a constant-coefficient stencil would match one pair per grid line per round).  A round that forms
 *       no pair ends the matching (later rounds would change nothing).  Rows still unmatched stay single.
 *     numbering  the root of an aggregate is its smaller member; coarse ids are the ranks of the roots in ascending order.  Then
 *       B' = P^T B P by the Galerkin rules above (fine rows ascending, entries in stored order, double / complex double, rounded
 *       once to the value type, columns ascending, structural zeros kept).  The next pass runs on B'.
 *   One LEVEL from the matrix A_l of level l: up to `passes` passes; a pass whose product has a row of more than 64 distinct columns
 *     is dropped together with the passes after it (the entry never returns that error: it stops coarsening instead); the passes
 *     kept give the composed map agg (aggregates of at most 2^passes <= 8 rows) and A_{l+1} = the last kept product.  The level is
 *     not built and the hierarchy ends at level l when no pass is kept or when 5 * rows(l + 1) > 4 * rows(l) (coarsening below 0.8:
 *     a star, a diagonal matrix, positive off-diagonals only).  Coarsening repeats while a level has more than min_rows rows, at
 *     most 16 levels.  Padding rows belong to no aggregate.  Errors about diagonals name the level and the row.
 *   Restriction sums the members of an aggregate in ascending row order; prolongation reads e[agg[i]].
 * passes 0 ... 3 (0 = 3), strength theta in (0, 1] (0 = 0.25), smooth_steps, over_correction, min_rows as in the grid entry.
 * CGAMD_ERR_INVALID: passes outside 0 ... 3, strength negative, above 1 or not finite, and the grid entry's for the other three.
 * cgamd_solver_mg_level reports nx = rows, ny = nz = 0 for the levels of an algebraic hierarchy. */
int cgamd_solver_set_preconditioner_amg(cgamd_solver *s, int passes, double strength, int smooth_steps, double over_correction, int min_rows);
/* Development entry, same standing as cgamd_solver_mg_level_matrix: the map level -> level + 1 of the hierarchy in force, `rows of the
 * level` ints to the host, *n_coarse = rows of the next level (either pointer may be NULL); also serves a grid hierarchy (the box
 * map).  CGAMD_ERR_INVALID on the coarsest level; synchronises. */
int cgamd_solver_mg_aggregates(cgamd_solver *s, int level, int *agg_host, int *n_coarse);
/* ---- Multigrid: the kernels (csrc/multigrid.hip, csrc/amg.hip) ----
 * Development entries (tests; same standing as the cgamd_mixed_* and cgamd_projection_* kernel entries): the three kernels of the
 * V-cycle and the scan of the setup as the hierarchy launches them, thin wrappers over the same launch functions, and what a handle's
 * hierarchy holds per level.  All pointers of the stateless entries are DEVICE pointers and free, as are the leading dimensions; a
 * call runs on the ctx stream and is synchronised.  CGAMD_ERR_INVALID, judged in this order and before the context is looked at: a
 * mode outside 0 .. 2, a null pointer that the call needs, a bad size / nRHS (negative size, nRHS < 1, a grid dimension < 1, n_coarse
 * that is not the number of boxes), a leading dimension below the size, a dtype outside the four value types, then ctx == NULL.  A
 * size of 0 launches nothing.
 * ARITHMETIC of all three: every operation is ONE IEEE operation in the value type T (no contraction into a multiply-add); complex
 * values go by components, vmul(a, b) = (ar br - ai bi, ar bi + ai br), a scale by c0, c1 or omega multiplies both components by the
 * coefficient ROUNDED TO THE REAL TYPE of T first.  No reductions across threads: every output element is one thread's own sequence,
 * so the bits do not depend on the launch geometry.  Column r of a vector starts at r * ld; dinv is shared by the columns.
 * NO LANE AT OR BEYOND `size` of any column is read or written (padding lanes between size and ld keep their bytes).
 * cgamd_mg_smooth_step: one Chebyshev step per lane i < size of every column, in this order:
 *     res = b[i]                      mode 0 (x = 0 on entry; w is NOT READ and may be NULL, x is NOT READ)
 *     res = b[i] - w[i]               modes 1 and 2 (w = A x)
 *     t   = vmul(dinv[i], res)        the complex product by components
 *     t   = c1 * t                    by components
 *     t   = c0 * d[i] + t             mode 2 only: the scaled d is the LEFT operand; d is NOT READ in modes 0 and 1
 *     d[i] = t                        only when store_d != 0: with store_d == 0, d is NOT WRITTEN (and may be NULL unless mode is 2)
 *     x[i] = t (mode 0) or x[i] + t   (modes 1 and 2)
 *   b, w and dinv are only read.  c0 is ignored in modes 0 and 1.
 * cgamd_mg_restrict: per coarse row I < n_coarse of every column: s = +0; for every fine row i of aggregate I, ASCENDING,
 *   s = s + (b[i] - w[i]); bc[I] = s; t = c1 * vmul(dinv_c[I], s); xc[I] = t; dc[I] = t only when store_d != 0 (else dc is NOT WRITTEN
 *   and may be NULL).  members == NULL: the box map of the nx x ny x nz grid (n_coarse = ceil(nx / 2) ceil(ny / 2) ceil(nz / 2); the
 *   rows of a box ascend as x fastest, then y, then z).  Otherwise members holds 8 ints per coarse row, fine rows ascending, -1 behind
 *   the last (a list of exactly 8 has no -1), read as two 16-byte loads: the pointer must be 16-byte aligned; nx names the number of
 *   fine rows (ny, nz unused) and every member must lie in [0, nx).  Fine rows in no aggregate are not read; b, w, dinv_c, members are
 *   only read.  ld_f >= fine rows, ld_c >= n_coarse.
 * cgamd_mg_prolong: x[i] = x[i] + omega * e[agg(i)] (by components) for i < n_fine of every column; nothing at or beyond n_fine.
 *   agg == NULL: the box map of the grid (n_fine <= nx ny nz, ld_c >= the number of boxes).  Otherwise agg holds n_fine ints, the
 *   coarse row of every fine row (nx, ny, nz unused; ld_c >= 1 is all that can be judged).  e and agg are only read.
 * cgamd_mg_scan: a[0 .. n - 1] counts (non-negative ints) -> exclusive prefix sums in place, a[n] = the total; integer sums, exact.
 *   One work-group of 1024 threads, thread t takes the chunk [t ceil(n / 1024), (t + 1) ceil(n / 1024)) cut at n.  A total above
 *   2^31 - 1: *overflow = 1, a[n] = 2^31 - 1 and every prefix is clamped to 2^31 - 1; otherwise *overflow is NOT WRITTEN (the caller
 *   presets it to 0).  Nothing behind a[n] is touched. */
int cgamd_mg_smooth_step(cgamd_ctx *ctx, int dtype, int mode, int size, long long ld, int nRHS, const void *dinv, const void *b,
                         const void *w, void *d, void *x, double c0, double c1, int store_d);
int cgamd_mg_restrict(cgamd_ctx *ctx, int dtype, int nx, int ny, int nz, const int *members, int n_coarse, long long ld_f, long long ld_c,
                      int nRHS, const void *b, const void *w, void *bc, const void *dinv_c, void *xc, void *dc, double c1, int store_d);
int cgamd_mg_prolong(cgamd_ctx *ctx, int dtype, int nx, int ny, int nz, const int *agg, int n_fine, long long ld_f, long long ld_c, int nRHS,
                     const void *e, void *x, double omega);
int cgamd_mg_scan(cgamd_ctx *ctx, int n, int *counts_to_ptr, int *overflow);
/* On a handle with a hierarchy in force (CGAMD_ERR_STATE without one, CGAMD_ERR_INVALID for a NULL handle or pointer, a level that does
 * not exist, or while the handle's stream is being captured); both synchronise.
 * cgamd_solver_mg_level_state, shaped like cgamd_solver_step_state (cap_values = values out_host holds; *count is set even when the
 *   capacity is too small, CGAMD_ERR_INVALID then).  which: 0 five ints -- n, the rows the level's kernels work on (level 0: with the
 *   padding rows), nu, the rows of the level, the leading dimension of its vectors, its smoothing steps (8 on the coarsest), 1 for an
 *   algebraic hierarchy; 1 dinv, n values of the handle's type (the padding rows of level 0 are +0); 2 / 3 c0[k] / c1[k], k <
 *   steps, as the doubles the launches are given (they round them to the real type; c0[0] = 0 is never read); 4 the member lists of the
 *   level's aggregates, 8 ints per row of the next level (CGAMD_ERR_INVALID for a grid hierarchy and for the coarsest level).
 *   The hierarchies of a batched handle: 1 is nSystems * ld values, system r at r * ld; 2 / 3 are steps * nSystems doubles, the
 *   coefficient of (step k, system r) at k * nSystems + r.
 * cgamd_solver_mg_level_spmv: w = A_level x exactly as the cycle launches it -- the level's own plan, n rows, the level's leading
 *   dimension ld for x and w -- on caller vectors of nRHS * ld values (device pointers).  cgamd_last_spmv_form afterwards reports
 *   what ran on that level.
 * The launch chain of one cycle, L = the last level, s_l = steps of level l (every smoothing step works on n rows, restriction on the
 * nu rows of level l + 1, prolongation on the nu rows of level l):
 *   down, l = 0 .. L:  l == 0: smooth_step mode 0 (x = z, b = r, store_d = s_0 > 1);  for k = 1 .. s_l - 1: w = A_l x, smooth_step mode 2
 *     (c0[k], c1[k], store_d = 1);  l < L: w = A_l x, restrict into level l + 1 (c1[0] of level l + 1, store_d = s_{l+1} > 1);
 *   up, l = L - 1 .. 0:  prolong (omega = over_correction), w = A_l x, smooth_step mode 1 (c1[0], store_d = s_l > 1), then the
 *     steps k = 1 .. s_l - 1 as above. */
int cgamd_solver_mg_level_state(cgamd_solver *s, int level, int which, void *out_host, long long cap_values, long long *count);
int cgamd_solver_mg_level_spmv(cgamd_solver *s, int level, const void *x_dev, void *w_dev);
/* where the preconditioner in force came from -- 0: none; 1: the caller's arrays (the three array entries above, and
 * cgamd_solver_set_preconditioner_batched); 2: the matrix, built on the device; 3: the matrix, extracted on the device but factored by
 * the host route (long segments; never on a batched handle) */
int cgamd_solver_preconditioner_source(cgamd_solver *s);
/* convenience: set_rhs + iterate + get_x (+ history if non-NULL, (nIterations+1)*nRHS values), host arrays */
int cgamd_solver_solve(cgamd_solver *s, const void *b, void *x, int nIterations, void *history);
/* the solver's SpMV (optionally fused with the d.q partial reduction) on caller vectors -- bench/profiling */
int cgamd_solver_spmv(cgamd_solver *s, const void *x, void *y, int fused_dot);
/* Development entries (tests of the SpMV forms; not part of the interface).
 * cgamd_last_spmv_form: what the CALLING THREAD's most recent SpMV launch (cgamd_solver_spmv, cgamd_spmv, an iteration's SpMV) really
 * launched, recorded where the kernel is launched.  Writes min(n_out, 10) ints and returns that count (negative: error):
 * [0] family: 0 generic stream, 1 row-block, 2 value-coded (vc), 3 value-coded pipelined (vcp), 4 chunked, 5 grouped SpMM, 6 batched (a matrix per right-hand side:
 * [2] batch length of the row walk, [7] 1 = the any-CSR form that reads the matrix per row), 9 split long rows (CGAMD_SPLIT_LONG_ROWS:
 * [2], [3] and [8] are the body's), -1 none yet;
 * [1] 16-byte loads (VEC); [2] batch length of the row walk / lanes per row (chunked) / right-hand sides per register group (SpMM);
 * [3] index encoding: 0 aCols, 8, 16 bits; [4] value encoding: 0 aValues, 1 code stream of its own, 2 joint (offset, value) codes;
 * [5] non-temporal matrix loads; [6] fused d.q; [7] wide (one work-group per row block AND right-hand side); [8] grid.x;
 * [9] d.q partials written per right-hand side (0 when not fused). */
int cgamd_last_spmv_form(int *out, int n_out);
/* Waits for the handle's stream and copies the d.q partials of its last fused SpMV to the host: [nRHS][*per_rhs] accumulators
 * (double; two doubles for the complex types), cap_values = accumulators `out_host` holds.  *per_rhs is set even when the
 * capacity is too small (CGAMD_ERR_INVALID then). */
int cgamd_solver_dot_partials(cgamd_solver *s, void *out_host, long long cap_values, int *per_rhs);
/* Development entries of the same standing (tests of the vector and scalar steps of an iteration; not part of the interface).  Neither
 * launches a kernel or changes the handle; both return CGAMD_ERR_INVALID while the handle's stream is being captured, and for handles
 * that run the tridiagonal preconditioner (their steps launch with grids of their own, not recorded).  A handle that keeps its block
 * row-major is refused by cgamd_solver_step_plan (cgamd_solver_rowmajor_plan describes its launches) and served by
 * cgamd_solver_step_state once cgamd_solver_layout() is 1: the r.r partials are [nRHS][rowmajor plan 8], there are no r.z partials and
 * no rho buffer (which 1 and 5: CGAMD_ERR_INVALID); cgamd_solver_dot_partials reports [nRHS][rowmajor plan 6] for it.
 * cgamd_solver_step_plan: what the vector and scalar launches of this handle use NOW, read from the fields the launch sites read.
 * Writes min(n_out, 11) ints and returns that count (negative: error): [0] working size n (rows including appended ones), [1] leading
 * dimension of the handle's vectors, [2] r.r / r.z partials per right-hand side (grid.x of the vector launches), [3] d.q partials per
 * right-hand side as the SpMV writes them (a CGAMD_UNFUSED handle sums the [2] partials of its own dot launch instead, see [7]), [4] / [5] order of the prologue sums over the d.q / r.r partials: 0 thread-strided, K > 0 member-blocked, K
 * consecutive partials per thread, [6] alpha folded into the r update's prologue, [7] the two-level cg_alpha2 is the alpha launch (the
 * launcher's rule, restated: not folded and at least 16384 partials to sum),
 * [8] 16-byte packs (0: the scalar form), [9] the streaming hints (vec_nt) the launchers resolve, [10] iterations per deferred x update
 * of a captured group (1: every iteration).
 * cgamd_solver_step_state: waits for the handle's stream and copies one piece of the iteration's state to the host.  which: 0 the r.r
 * partials, 1 the r.z partials (diagonal preconditioner), [nRHS][plan 2] accumulators (double; two doubles for the complex types);
 * 2 alpha, 3 beta, 4 delta: nRHS values of the handle's type; 5 the rho parity buffer, [2][nRHS] values; 6 the iteration counter, one
 * int.  cap_values = values `out_host` holds; *count is set to the number the state has even when the capacity is too small
 * (CGAMD_ERR_INVALID then). */
int cgamd_solver_step_plan(cgamd_solver *s, int *out, int n_out);
int cgamd_solver_step_state(cgamd_solver *s, int which, void *out_host, long long cap_values, long long *count);
/* Of the same standing: what the launches of the row-major loop use NOW (cgamd_solver_layout() == 1; any other handle:
 * CGAMD_ERR_INVALID), read from the functions and fields the launch sites read.  Writes min(n_out, 17) ints and returns that count
 * (negative: error): [0] working size n, [1] real columns of the block (complex64: 2 nRHS), [2] values a lane loads per non-zero (NH),
 * [3] / [4] K-steps per quad and round (TQ: 5 or 8) of the SpMM instance with / without the fused d.q, [5] strips of 16 rows,
 * [6] / [7] work-groups of the SpMM launch with / without the fused d.q ([6] = d.q partials per right-hand side as the kernel lays them
 * out), [8] grid of the rm_dot / rm_axpy_dot / rm_aypx_x launches (r.r partials per right-hand side), [9] / [10] rm_axpy_dot / rm_aypx_x
 * launch their streaming (NT) form, [11] / [12] order of the sums over the d.q / r.r partials as in step_plan [4] / [5], [13] / [14] XCDs
 * (of 8) whose sweep paces itself in the launch with / without the fused d.q (0: unpaced), [15] steps a paced wave may lead by,
 * [16] d.q partials per right-hand side the alpha launch sums (the handle's field; equals [6]). */
int cgamd_solver_rowmajor_plan(cgamd_solver *s, int *out, int n_out);
/* Of the same standing: the form the SpMV of this handle's launched loop WILL take -- the launcher's own decision, asked without a
 * launch -- in the layout of cgamd_last_spmv_form.  fused: with the d.q partials (what every loop but CGAMD_UNFUSED launches) or
 * without.  Writes min(n_form, 10) ints to `form` and returns that count (negative: error).  inputs (may be NULL): min(n_inputs, 62)
 * ints, everything the decision read -- the call (value and accumulator size, n, nRHS, alignments, whether the codes belong to the
 * handle's arrays, fused, row-block list), the plan (pointers as 0 / 1) and the tuning keys, in the order of kSpmvFormInputNames
 * (csrc/spmv_form.cpp).  cgamd_solver_joint_codes, _row_codes, _row_pairs, _row_pipe, _spmv_schedule, _spmv_moved_bytes and
 * _iter_moved_bytes are read off this form. */
int cgamd_solver_spmv_form(cgamd_solver *s, int fused, int *inputs, int n_inputs, int *form, int n_form);
/* SpMM on the matrix cores (BASELINE config 4, "MFMA tall-B tile path"): Y[size][nRHS] = A * X[size][nRHS] with
 * the right-hand-side block in ROW-MAJOR layout (element i of RHS r at [i*nRHS + r]); f64 with nRHS = 16 or 32, f32 with 16, 32
 * or 64, complex64 with 16 or 32; any CSR matrix.  Solvers created with such a width keep their vectors in this layout
 * internally and run this kernel in the CG loop (cgamd_solver_layout() == 1); set_rhs / get_x / solve still take and
 * return the reference's RHS-major blocks.  cgamd_transpose converts between the two: out[c*rows + r] = in[r*cols + c]. */
int cgamd_solver_spmm_rowmajor(cgamd_solver *s, const void *x, void *y, int nRHS);
/* 0: the handle's vectors (cgamd_solver_vector) are RHS-major [nRHS][size]; 1: row-major [size][nRHS] (decided by the
 * last cgamd_solver_set_rhs) */
int cgamd_solver_layout(cgamd_solver *s);
/* launches per iteration of the loop cgamd_solver_iterate runs for this handle: 0 = the resident loop (small systems: every
 * iteration of a call of at least `resident_min` iterations inside ONE launch, csrc/resident.hip), 1 = its chip-wide form
 * (one launch per call of at least `resident_wide_min` iterations as well; shorter calls take the launched loops of the same handle,
 * which return the same bits), 2 / 3 / 4 / 5 = the
 * loops of DESIGN.md section 4, 8 = the reference's op structure (CGAMD_UNFUSED); negative: error */
int cgamd_solver_loop_launches(cgamd_solver *s);
/* L >= 2: the handle's captured runs of 8 iterations (three / four-launch loop, no preconditioner) bring x up to date once per L
 * iterations instead of in every one: x is read by nothing inside the loop, so the directions of a group are kept and its last
 * iteration applies all L updates in iteration order.  Every call returns with nothing pending and x, r, d,
 * the scalars and the history bit-identical to L = 1.  By default (L = 4) on the four-launch loop of large systems (more than 2048 d.q
 * partials, i.e. beyond 524k rows) that no resident loop takes; costs (L - 2) * size * nRHS values of device memory beside the
 * handle's vectors -- a handle that cannot have them runs L = 1.  1 = x is updated in every iteration; negative: error */
int cgamd_solver_x_lag(cgamd_solver *s);
/* > 0: this handle's single-RHS SpMV reads one-byte column codes instead of aCols (4 -> 1 byte of index traffic per non-zero),
 * the value is the number of distinct (column - row) offsets of the matrix (at most 256; stencil / structured-grid FE matrices
 * have 5 to 27).  Built at create / reload for matrices above 32 MB (tuning key "index_codes_min_mb"; smaller systems run
 * the resident or two-launch loops; "index_codes" 0 disables).  Exact: the kernel rebuilds the same column, results do not change by a bit.
 * 65536: the matrix has more offsets than that, and the SpMV reads 16-bit columns relative to the first column of every 256-row block
 * (2 index bytes per non-zero; any matrix whose row blocks span fewer than 65 536 columns each: banded random patterns, meshes in a
 * bandwidth-reducing order, what Matrix-Market files hold; tuning key "index_codes16" 0 disables).  Exact like the one-byte form.
 * 0: the kernel reads aCols as the reference's does (kernel/real/spmv.cl:21-27). */
int cgamd_solver_index_codes(cgamd_solver *s);
/* distinct matrix entries behind the one-byte VALUE codes of the handle's single-RHS SpMV (matrices of at most 256 distinct entries
 * that also run on one-byte column codes: 2 bytes per non-zero from memory, same bits); 0 = the SpMV reads aValues.
 * (cgamd_tune("dev.value_codes", 0) turns the form off for A/B runs.)  After a cgamd_solver_refresh_values that rewrote the
 * dictionaries in place (cgamd_solver_last_refresh() == 1) this accessor, cgamd_solver_joint_codes and cgamd_solver_row_codes report
 * the dictionary ENTRIES IN USE, which exceed the number of distinct values / pairs / patterns when classes of values have merged. */
int cgamd_solver_value_codes(cgamd_solver *s);
/* > 0: the SpMV reads ONE byte per non-zero that names the (column offset, value) pair -- matrices with at most 256 distinct pairs whose
 * longest row fits one batch of the row walk (constant-coefficient stencils: as many pairs as offsets); the value is the number of
 * pairs.  0: it reads the column codes and the value codes (2 bytes), or aCols / aValues. */
int cgamd_solver_joint_codes(cgamd_solver *s);
/* > 0: the SpMV reads ONE byte per ROW that names the row's pattern -- its (column offset, value) pairs in stored order -- instead of a
 * byte per non-zero and the row pointers: matrices that run on joint codes, above 32 MB (cgamd_tune("dev.row_codes_min_mb")), with rows
 * of at most 7 entries and at most 256 distinct patterns (the 7-point Laplacian has 27, the 5-point one 9); the value is the number of
 * patterns.  Same products in the same order: same bits.  0: another form runs (cgamd_tune("dev.row_codes", 0) keeps the joint one).
 * cgamd_last_spmv_form reports it as family 7, [2] batch length, [3] 8, [4] 3. */
int cgamd_solver_row_codes(cgamd_solver *s);
/* the number of row blocks (1, 2 or 4 of the 4 a work-group takes) whose gathers the handle's row-coded SpMV keeps in flight per wave:
 * the default, or what cgamd_tune("dev.row_pipe") forced when the handle was created -- the depth the launch goes out with: a handle on
 * the row-PAIR form keeps at most 2 of its two passes in flight and reports that.  Every depth forms the same bits.  0: the handle
 * does not run the row-coded form. */
int cgamd_solver_row_pipe(cgamd_solver *s);
/* the number of row-PAIR patterns of a handle whose row-coded SpMV takes two rows per lane: one byte per pair of rows (2p, 2p + 1)
 * names the union of the two rows' slots, and one 16-byte load per slot serves both rows.  Same products in the same order per row:
 * same bits.  0: the row form (or another) runs -- cgamd_tune("dev.row_pairs", 0), a matrix below dev.row_pairs_min_mb, more than
 * 256 pair patterns, or a pair whose union needs more than 8 slots.  cgamd_last_spmv_form reports the pair form as family 8; a
 * launch whose vectors are not 16-byte aligned runs the row form (family 7). */
int cgamd_solver_row_pairs(cgamd_solver *s);
/* how the handle's row- or pair-coded SpMV deals its super blocks (1024 rows, one work-group each) to the eight XCDs.  *kind 1: the
 * PLANE-MATCHED table -- super block s runs on XCD floor(8 frac(centre(s) / unit)), every XCD's blocks in ascending order, so rows r and
 * r + unit (the neighbours across the largest stride: a z plane of a 3-D grid) meet in one XCD's L2 and their line of x is fetched
 * once; *kind 0: the block-cyclic schedule of the tuning key "spmv_cycle".  *grid: the work-groups of a launch (0: the handle runs
 * neither form); *unit_rows: the largest |column - row| among the handle's row patterns (0 likewise).  Which work-group computes a
 * row enters no result: same bits under either kind.  cgamd_tune("dev.spmv_plane", 1 / 0) forces the table or the cycle for handles
 * created afterwards (1: for any unit of at least one row, however unevenly the table loads the XCDs -- a unit of exactly one super
 * block puts every block on one XCD; a development setting); -1 restores the default rule: the table where the unit is at least 8
 * super blocks (3-D grids), the matrix above 256 MB and the longest XCD list at most 2 % above an eighth of the super blocks, else the
 * cycle (a third less read traffic, 1 to 2 % of an iteration).  Any out pointer may be NULL. */
int cgamd_solver_spmv_schedule(cgamd_solver *s, int *kind, int *grid, long long *unit_rows);
int cgamd_transpose(cgamd_ctx *ctx, int dtype, int rows, int cols, const void *in, void *out);
/* algorithmic HBM bytes of one SpMV / one CG iteration of this solver (SURVEY §8d formulae: 14 vector passes for the
 * reference's op structure, 11 for its "fused minimum"; the default loop here moves 10) */
long long cgamd_solver_spmv_bytes(cgamd_solver *s);
long long cgamd_solver_iter_bytes(cgamd_solver *s, int fused);
/* the bytes this handle's own kernels move per SpMV / per iteration of its launched loop: index bytes per non-zero as the SpMV
 * reads them (1 with one-byte column codes, 2 with 16-bit block-relative columns, 4 with aCols) and the loop's own vector passes
 * (10 by default; (9 L + 1) / L in the steady state of a handle with cgamd_solver_x_lag() = L >= 2).  This is the figure a roofline FRACTION is priced on; the SURVEY 8(d) figures above are the
 * reference's CSR byte model (an "effective" rate). */
long long cgamd_solver_spmv_moved_bytes(cgamd_solver *s);
long long cgamd_solver_iter_moved_bytes(cgamd_solver *s);

/* ---- Long rows (CGAMD_SPLIT_LONG_ROWS; csrc/long_rows.hip).  Graph Laplacians with a few high-degree vertices, circuit matrices with
 * supply nets and grid systems with one coupled unknown have a few rows of thousands to millions of entries.  The plan chooses ONE
 * kernel per matrix from the largest slice span of any 256-row block, so one such row costs every row the block forms, and the row
 * itself is walked by one work-group.  With the flag the handle's single-right-hand-side SpMV takes a fourth way:
 *   HEAVY RULE.  A 256-row block is heavy when any of its 8-row slices (rows 8 k .. 8 k + 7 of the block) spans more than
 *   48 KB / (sizeof(value) + 4) entries, the span measured from aPointers[first row] rounded down to a multiple of 4 to
 *   aPointers[last row + 1] -- exactly the blocks that even the chunked form with 32 lanes per row cannot stage.  The rule reads the
 *   row pointers only.  (cgamd_tune "dev.long_row_bytes" lowers the 48 KB for tests.)
 *   Every other block runs the row-block or chunked kernel, chosen from THEIR spans by the rules of an unflagged handle, on aCols;
 *   the rows of those blocks have the bits an unflagged handle of the matrix without the heavy blocks would give them.
 *   A heavy block's span is cut into segments of 2048 entries ("dev.long_row_segment": another multiple of 4; clamped so that a
 *   segment's values and columns fit 128 KB), one work-group each; a second launch of one work-group per heavy block completes the
 *   rows and forms the block's d.q partial.  Nothing of the matrix is copied; no atomics, no spins.
 *   SUMMATION ORDER of a row of a heavy block: inside each segment the row's entries ("piece") are summed from +0 in stored order by
 *   one lane when the piece has at most 64 entries (a row that lies inside one segment and is that short has the bits of every
 *   one-lane form), else by 64 lanes -- lane l adds entries l, l + 64, ... from +0, then v[l] += v[l + off], off = 32, 16, 8, 4, 2, 1,
 *   lane 0; a row that crosses segment edges is the sum of its pieces in ascending segment order from +0.  All in the value type.
 *   Results are the same from run to run, with and without hipGraph replay, and however a solve is cut into iterate() calls.
 * The flag applies to cgamd_solver_create handles with nRHS == 1 whose aValues and aCols are 16-byte aligned and whose plan would
 * otherwise end at the generic stream kernel because of its spans.  Everywhere else -- batched handles, several right-hand sides,
 * "dev.generic_spmv" = 1, misaligned borrowed arrays, a matrix without heavy blocks -- it changes nothing, by a bit or by a launch,
 * and the query reports zeros.  CGAMD_HERMITIAN handles are served.  cgamd_dist_* and cgamd_mixed_* do not take the flag.  Such a
 * handle runs the launched loops (plain, iterate_until, diagonal / line / multigrid PCG, CGAMD_NO_GRAPH); the resident, chip-wide
 * and two-launch loops need the one-kernel row-block plan and do not take it, and it builds no column or value codes.
 * cgamd_solver_refresh_values: the kernels read the values live, the lists depend on the row pointers only and stay.
 * cgamd_last_spmv_form reports family 9 with [2] the body's batch length or lanes per row, [3] its index encoding, [8] its grid and
 * [9] one partial per 256-row block.  The byte model prices the matrix once plus the piece scratch written and read.
 * cgamd_solver_long_rows: writes min(n_out, 6) ints and returns that count (negative: error): [0] heavy blocks, [1] segments,
 * [2] entries per segment, [3] the body's kind (5 row-block, 7 chunked, 0 no regular block), [4] its lanes per row, [5] scratch bytes;
 * all 0 where the flag is not set or does not apply. */
int cgamd_solver_long_rows(cgamd_solver *s, int *out, int n_out);

/* ---- Mixed precision (csrc/mixed.cpp, csrc/mixed.hip): an fp64 / complex128 answer at close to the fp32 / complex64 loop's byte rate.
 * The loops are bound by bytes and most of them are vectors; fp32 alone stalls near 1e-6 ||b||.  Here the recurrence runs in the lo
 * type on the INNER handle while x and the true residual r = b - A x are kept in the hi type on the OUTER handle; whenever the inner
 * residual has dropped by `delta` the inner x is added into the outer x, the true residual is recomputed, rounded down and handed
 * back through cgamd_solver_replace_residual -- the search direction is kept, so no Krylov space is thrown away (a restarted iterative
 * refinement took 1.3 - 1.7 x the fp64 iteration count on the Poisson systems tried, this scheme 1.0 - 1.17 x).
 * cgamd_mixed_create: dtype_hi CGAMD_F64 (lo: CGAMD_F32) or CGAMD_C128 (lo: CGAMD_C64); any other dtype: CGAMD_ERR_INVALID.  flags:
 * CGAMD_NO_GRAPH and CGAMD_MATRIX_ON_DEVICE; any other flag (CGAMD_UNFUSED, CGAMD_HERMITIAN, ...): CGAMD_ERR_INVALID.  Both are judged
 * before a device is touched.  The outer handle is an ordinary handle of the hi type (with CGAMD_MATRIX_ON_DEVICE it borrows the
 * caller's arrays); the inner handle is an ordinary lo handle on the values rounded once, on the device, at create -- a copy the mixed
 * handle owns.  CHANGING THE BORROWED VALUES NEEDS A NEW MIXED HANDLE: the lo copy does not follow them (no refresh_values here).
 * Preconditioners go on the inner handle through the existing entries, cgamd_solver_set_preconditioner(cgamd_mixed_inner(m), ...) and
 * _jacobi; the handles cgamd_mixed_outer / _inner return belong to the mixed handle and die with it.
 * cgamd_mixed_solve: b and x hold nRHS * size values of the hi type at stride `size`, host (on_device = 0) or device memory; x is
 * in / out: the initial guess, then the solution.  tol: nTol = 1 or nRHS positive values (host).  Per right-hand side r:
 *   1. r_hi = b - A x_hi and delta = r_hi . r_hi, the bits of cgamd_solver_set_rhs(outer, b, x_hi); res_r = sqrt|delta| (the
 *      unconjugated measure cgamd_solver_iterate_until uses).  !(res_r >= tol_r): done, status 0 -- at the start: x is x0 unchanged,
 *      iterations 0; a non-finite res_r: status 2.  s_r = 2^ilogb(sqrt(sum |r_hi,i|^2)), fixed for the whole solve.
 *   2. first segment: cgamd_solver_set_rhs(inner, LO(r_hi / s_r)); 3. later ones: cgamd_solver_replace_residual(inner, LO(r_hi / s_r)).
 *   4. cgamd_solver_iterate_until(inner, min(budget left, maxSegment), t, ...) with t_r = max(delta * start_r, tol_r / s_r), start_r =
 *      sqrt|history row 0| of the segment.  A right-hand side that is done gets t_r = DBL_MAX: it stops after one iteration and is
 *      masked out of step 5 (its x is not touched again).
 *   5. x_hi += s_r * HI(x_lo) (exact product, one rounding), then step 1 with the new x_hi.  iterations[r] adds up the column's
 *      iterations of the segments in which it was open; *replacements counts the segments.
 *   6. The solve ends when every right-hand side is done, or when maxIterations is used up -- counted as the sum of the inner
 *      handle's iteration counts over the segments; right-hand sides still open then have status 1, x is the accumulated iterate
 *      and resnorm its TRUE residual norm.  resnorm[r] is always sqrt|r_hi . r_hi| of the x returned.
 * delta: in [0, 1), 0 = 0.1.  maxSegment: 0 = no cap.  checkEvery: as in cgamd_solver_iterate_until; the result does not depend on
 * it, and is the same bits from run to run.  The host synchronises once per segment, beside the waits of cgamd_solver_iterate_until.
 * Errors: what the inner handle does not serve (a tridiagonal / line preconditioner, a row-major width) is returned as the
 * CGAMD_ERR_STATE of cgamd_solver_replace_residual before anything is touched; x is unchanged on every error.  Not served: Hermitian,
 * batched and row-partitioned handles, cgamd_solver_refresh_values on either handle.
 * cgamd_mixed_scales: s_r of the last solve, nRHS doubles. */
typedef struct cgamd_mixed cgamd_mixed;
int cgamd_mixed_create(cgamd_ctx *ctx, int dtype_hi, int size, long long nnz, const void *aValues_hi, const int *aPointers,
                       const int *aCols, int nRHS, int flags, cgamd_mixed **out);
int cgamd_mixed_destroy(cgamd_mixed *m);
cgamd_solver *cgamd_mixed_outer(cgamd_mixed *m);
cgamd_solver *cgamd_mixed_inner(cgamd_mixed *m);
int cgamd_mixed_solve(cgamd_mixed *m, const void *b, void *x, int on_device, const double *tol, int nTol, int maxIterations, double delta,
                      int maxSegment, int checkEvery, int *iterations, double *resnorm, int *status, int *replacements);
int cgamd_mixed_scales(cgamd_mixed *m, double *scales);
/* ---- Mixed precision: the kernels (csrc/mixed.hip).  The four streaming kernels between the hi and the lo side as stateless
 * entries, the launches cgamd_mixed_solve itself makes.  All pointers are DEVICE pointers; a call is enqueued on the ctx stream and
 * does not synchronise.  dtype_hi: CGAMD_F64 (lo: float) or CGAMD_C128 (lo: complex64).  Every operation is real and component-wise:
 * a column of `size` values is m = size * R real lanes, R = 1 (CGAMD_F64) or 2 (CGAMD_C128).  Column r of an array starts r * ld
 * VALUES (not lanes) after its pointer; ld >= size.  The library is built with -ffp-contract=off: every product and every sum below
 * is one IEEE operation in double, every conversion to float one rounding to nearest-even with gradual underflow (a result below
 * 2^-126 is a float subnormal, not zero), overflow to +-inf, NaN to NaN, -0 to -0.
 * THE TWO FORMS.  A kernel runs its 16-byte form -- lanes 4 q .. 4 q + 3 of a column as one float4 and two double2 accesses, q <
 * m / 4, and the m % 4 lanes left as a scalar tail -- when every array pointer of the call is 16-byte aligned and, where nRHS > 1,
 * every leading dimension is a whole number of 16-byte packs (ld_hi * 8 R and ld_lo * 4 R both multiples of 16).  Otherwise the scalar
 * form runs, lane by lane.  The element-wise results are the same bits in both forms; the order of the norm's sum is not.
 * cgamd_mixed_accumulate: x_hi[i] = x_hi[i] + scale[r] * (double)x_lo[i] per lane, i < m, for the columns with mask[r] != 0: two
 * roundings at most -- the product, exact when scale[r] is a power of two and the product neither overflows nor underflows, and the
 * sum.  A column with mask[r] == 0 is NEITHER READ NOR WRITTEN, on either side.  Nothing beyond lane m of a column is touched.
 * cgamd_mixed_round_down: r_lo[i] = (float)(r_hi[i] * inv_scale[r]), i < m: the product rounds once in double (not at all for a power
 * of two in range), the conversion once.  The lo side's padding, values size <= i < ld_lo of EVERY column (the last one too: r_lo
 * holds nRHS * ld_lo values), is written as +0.  The hi side is only read.
 * cgamd_mixed_norm2: out[r] = sum of v[i]^2 over the m lanes of column r (the conjugated norm, re^2 + im^2), in double, in a fixed
 * order: G = cgamd_mixed_norm2_grid(dtype_hi, size) = min(1024, ceil(m / 4096)) work-groups of 256 threads per column.  Thread t of
 * work-group g starts from +0 and adds, with T = 256 g + t and S = 256 G: 16-byte form -- the quads q = T, T + S, ... < m / 4, the
 * four squares of a quad in lane order, then the tail lanes 4 (m / 4) + T (T < m % 4); scalar form -- the lanes T, T + S, ... < m.
 * Then the work-group's 256 values are added by the wave tree v[l] += v[l + off], off = 32 .. 1, per 64 lanes, and the four wave sums
 * as ((w0 + w1) + w2) + w3: partials[r * G + g].  One thread then adds the G partials of a column from +0 in index order: out[r].
 * No atomics: the same bits on every run.  partials: nRHS * G doubles, written in full.  cgamd_mixed_norm2_grid: 0 for a dtype_hi
 * that is not served or size < 1 (no device is touched).
 * cgamd_mixed_round_values: lo[j] = (float)hi[j] over count * R lanes, one rounding each; 16-byte form when both pointers are aligned.
 * size (count) == 0: CGAMD_OK, nothing is launched.  CGAMD_ERR_INVALID, judged in this order and before a device is touched: a NULL
 * array pointer, a leading dimension below size, a dtype_hi other than the two, size < 0 or nRHS < 1, ctx == NULL. */
int cgamd_mixed_accumulate(cgamd_ctx *ctx, int dtype_hi, int size, void *x_hi, long long ld_hi, const void *x_lo, long long ld_lo,
                           const double *scale, const int *mask, int nRHS);
int cgamd_mixed_round_down(cgamd_ctx *ctx, int dtype_hi, int size, const void *r_hi, long long ld_hi, void *r_lo, long long ld_lo,
                           const double *inv_scale, int nRHS);
int cgamd_mixed_norm2_grid(int dtype_hi, int size);
int cgamd_mixed_norm2(cgamd_ctx *ctx, int dtype_hi, int size, const void *v, long long ld, int nRHS, double *partials, double *out);
int cgamd_mixed_round_values(cgamd_ctx *ctx, int dtype_hi, long long count, const void *hi, void *lo);

/* one-call typed solve on host arrays: cg() generalised to all four dtypes, with history and status */
int cgamd_cg(int dtype, int size, long long nnz, const void *aValues, const void *b, const int *aPointers,
             const int *aCols, void *x, int nRHS, int nIterations, void *history, int device);
/* Wall-clock split of the calling thread's last cgamd_cg() / cg() call, in milliseconds:
 * [0] device state (context, allocations, plan; or the cache check), [1] matrix upload + validation, [2] right-hand side
 * upload + setup kernels, [3] iterations (enqueue + wait), [4] solution download, [5] 1.0 when the call reused the
 * thread's cached device state.  cgamd_cg keeps one context + handle per calling thread and reuses them when dtype,
 * size, nonZeros, nRHS and device repeat (the reference rebuilds everything per call, clcg.c:142-214; the call itself
 * stays stateless: the matrix is re-uploaded every time).  cgamd_cg_release_cache() frees the calling thread's cache;
 * environment CGAMD_CG_NO_CACHE=1 disables it. */
int cgamd_cg_last_timing(double *ms6);
int cgamd_cg_release_cache(void);

/* ---- synthetic matrix generators, written straight into device memory -----
 * 7-point 3-D Laplacian (x fastest), Dirichlet, diag 6 / off-diag -1 (SURVEY §8d "M", "C5").
 * Generates global rows [row_begin,row_end) with GLOBAL column indices; canonical CSR.
 * Pass aPointers==NULL to query nnz of the slab via *nnz_out. */
int cgamd_gen_laplace3d(cgamd_ctx *ctx, int dtype, int nx, int ny, int nz, long long row_begin,
                        long long row_end, void *aValues, int *aPointers, int *aCols, long long *nnz_out);
/* 5-point 2-D Laplacian N x N, diag 4 / off-diag -1 (reference Poisson(), p_h-PY_C-CL.py:1642-1682) */
int cgamd_gen_poisson2d(cgamd_ctx *ctx, int dtype, int N, void *aValues, int *aPointers, int *aCols,
                        long long *nnz_out);

/* P1 finite-element Helmholtz matrices of the reference's drivers, Nhoriz x Nvert nodes, complex symmetric, 7 entries per interior
 * row (canonical CSR; dtype complex64 or complex128; values evaluated in complex double in the reference's operation order):
 *   cgamd_gen_helm_fe_var: helmFE_var(N, omega, C, rho, Nhoriz, Nvert) of helmFE_var.py:9-331 -- BASELINE config 3 is N = Nhoriz =
 *     Nvert = 500, omega = 12, C = 1, rho = 0.15.  C: (Nvert - 1) x (Nhoriz - 1) wave speeds, row-major, HOST doubles (NULL = all 1);
 *   cgamd_gen_local_rect:  local_rect(N, k, eps, eta, L, Nhoriz, Nvert) of p_h-PY_C-CL.py:1439-1639 -- the sub-domain matrices
 *     as_prec hands to cg().
 * Pass aPointers == NULL to query the number of non-zeros via *nnz_out. */
int cgamd_gen_helm_fe_var(cgamd_ctx *ctx, int dtype, int N, double omega, const double *C, double rho, int Nhoriz, int Nvert,
                          void *aValues, int *aPointers, int *aCols, long long *nnz_out);
int cgamd_gen_local_rect(cgamd_ctx *ctx, int dtype, int N, double k, double eps, double eta, double L, int Nhoriz, int Nvert,
                         void *aValues, int *aPointers, int *aCols, long long *nnz_out);

/* Right-hand sides of the reference's Helmholtz drivers on an N x N node grid (helmFE_var.py:333-389), written to device memory
 * as N * N values, entry (row, col) at row * N + col: kind 0 = rhs(N, k) (plane-wave boundary data; complex types only), 1 = rhsL(N, k)
 * (k^2 on the left boundary without its corners), 2 = rhsA(N, k) (k^2 on the four boundary lines: BASELINE config 3 uses rhsA(500, 12)). */
int cgamd_gen_rhs(cgamd_ctx *ctx, int dtype, int kind, int N, double k, void *b);

/* ---- Matrix-Market ingest (reference main.c:20-33 via BeBOP) ---------------
 * Reads a coordinate file (real/complex/integer/pattern x general/symmetric/hermitian/skew-symmetric),
 * expands symmetric storage, sums duplicates, converts 1-based -> 0-based CSR with sorted columns.
 * Values are returned as double (is_complex=0) or interleaved double pairs (is_complex=1).
 * Free the three arrays with cgamd_mm_free. */
int cgamd_mm_read(const char *path, int *size, long long *nnz, int *is_complex, double **values,
                  int **pointers, int **cols);
void cgamd_mm_free(void *p);

/* ---- row-partitioned multi-GPU CG (one process per GPU, RCCL over xGMI) ----
 * The host (torch.distributed) builds the partition plan; this library runs the loop.
 * See DESIGN.md "Multi-GPU" for the plan layout. */
typedef struct cgamd_dist cgamd_dist;
int cgamd_comm_unique_id(void *id128);      /* rank 0: 128 bytes to broadcast */
/* A peer may be the rank itself (periodic coupling inside one partition; also how a single GPU exercises the
 * exchange): its send list is then gathered into its own halo slots through ncclSend/ncclRecv to self. */
int cgamd_dist_create(cgamd_ctx *ctx, const void *id128, int rank, int nranks, int dtype,
                      int n_local, int n_halo, long long nnz_local, const void *aValues,
                      const int *aPointers, const int *aCols, /* device, cols in [0,n_local+n_halo) */
                      int n_peers, const int *peer_rank, const int *send_count, const int *recv_count,
                      const int *send_index /* device: concatenated local row ids to send */,
                      int flags, cgamd_dist **out);
int cgamd_dist_destroy(cgamd_dist *d);
int cgamd_dist_set_rhs(cgamd_dist *d, const void *b_local, const void *x0_local);   /* device pointers */
/* nIterations more iterations, asynchronous.  CGAMD_ERR_STATE without a cgamd_dist_set_rhs, and on a handle that
 * cgamd_dist_iterate_until has stopped (it stays stopped until the next cgamd_dist_set_rhs). */
int cgamd_dist_iterate(cgamd_dist *d, int nIterations);
/* Tolerance stop on the device for the row-partitioned handle: the single-right-hand-side case of cgamd_solver_iterate_until (the
 * reference's `tol` loop, p_h-PY_C-CL.py:1338-1369; PCG: helmFE_var.py:580-584).  COLLECTIVE IN MEANING: every rank makes the same
 * call with the same arguments.  The handle stops in the first iteration k >= 1 of such a call for which
 * !(sqrt|delta_k| >= tol), delta_k being the GLOBALLY reduced unconjugated r_k . r_k, exactly the value the history records -- with
 * a preconditioner still r.r, not rho; NaN stops; the test is evaluated in double.  The reduced value is bit-identical on every rank
 * (rank-ordered sums of the peer-to-peer rounds, one result of an RCCL all-reduce), so all ranks stop in the same iteration without a
 * further exchange.  After a stop cgamd_dist_get_x returns the local rows of the iterate of exactly the stopping iteration -- the bits
 * of set_rhs; iterate(its) on this handle's launched loop -- *iterations_run and cgamd_dist_iterations_done are its, and
 * cgamd_dist_history returns rows 0..its, bit-identical to a fixed-count run.  Without a stop *iterations_run is the handle's count
 * (iterations since cgamd_dist_set_rhs).  maxIterations == 0 returns the count at once.
 * The call synchronises, but never per iteration: it enqueues chunks of checkEvery iterations (0 = 8), copies one device word -- still
 * active: 1 / 0 -- asynchronously to pinned memory after each, and waits for the word of chunk c - 1 once chunk c is enqueued.
 * Iterations enqueued after the stop change nothing, so the result does not depend on checkEvery.  COMMUNICATION NEVER DEPENDS ON
 * THE STOP: after it every enqueued iteration still runs its halo push and wait, every all-reduce round (RCCL or mailbox slots) and
 * every epoch bump on every rank; only the writes of x, r, d, the scalars, the history and the counter are guarded, so no rank waits
 * for one that left early.  The call may follow cgamd_dist_iterate calls (their iterations are not examined again) and may be
 * repeated: until(a); until(b) leaves the bits of until(a + b).  A stopped handle stays stopped until the next cgamd_dist_set_rhs:
 * cgamd_dist_iterate returns CGAMD_ERR_STATE, a further cgamd_dist_iterate_until returns its at once, whatever the new tolerance.
 * Served: the RCCL loop and both peer-to-peer loops (four-launch and CGAMD_DIST_P2P_STAGED), with or without a preconditioner,
 * CGAMD_DIST_NO_OVERLAP, CGAMD_DIST_GRAPH (the guarded iterations run as plain launches).  A CGAMD_DIST_RESIDENT handle runs its
 * LAUNCHED loop in this call, as it does while a preconditioner is set; the slab loop has no stop, and its iterates are not the
 * launched loop's bit for bit, so "the bits of set_rhs; iterate(its)" there means iterate calls the launched loop serves.
 * CGAMD_ERR_INVALID: NULL d or iterations_run, tol not > 0 (NaN included), negative maxIterations or checkEvery.  CGAMD_ERR_STATE,
 * the handle untouched: no cgamd_dist_set_rhs; a CGAMD_DIST_SINGLE_REDUCTION handle (that loop runs another recurrence and a tail
 * launch per call; it has no guarded form).  A failed launch or a peer-to-peer time-out (cgamd_dist_p2p_error; CGAMD_ERR_COMM) ends
 * the call with that error, and the handle demands a fresh cgamd_dist_set_rhs. */
int cgamd_dist_iterate_until(cgamd_dist *d, int maxIterations, double tol, int checkEvery, int *iterations_run);
int cgamd_dist_iterations_done(cgamd_dist *d);   /* iterations since set_rhs; after a stop: the stopping iteration; negative: error */
int cgamd_dist_get_x(cgamd_dist *d, void *x_local);                                  /* device pointer */
int cgamd_dist_history(cgamd_dist *d, void *history, int max_entries);
int cgamd_dist_synchronize(cgamd_dist *d);
/* Preconditioned CG on the row-partitioned handle.  The preconditioner is RANK-LOCAL (block-Jacobi over the ranks): symmetric, positive
 * definite whenever A is, and applied without communication.  The three calls are collective in meaning -- every rank must make the
 * same one -- but local in execution: they do not communicate, so the CALLER makes sure that all ranks succeeded before anyone
 * iterates (ranks running different recurrences wait for each other's sums until the peer-to-peer time-outs; DistSolver.
 * set_preconditioner all-gathers the status).  They take effect at the next cgamd_dist_set_rhs: z0 = M^-1 r0, d = z0, rho0 = the
 * all-reduced r0.z0; rho = r.z then drives alpha and beta, and both sums of an iteration (r.z, r.r) travel in ONE all-reduce round.
 * cgamd_dist_history keeps returning r.r.  A failed call leaves the handle as it was; contracts otherwise as the cgamd_solver_*
 * entries of the same names.  Loops: the RCCL loop and both peer-to-peer loops, with or without CGAMD_DIST_GRAPH (a captured graph is
 * dropped when the preconditioner changes); a CGAMD_DIST_RESIDENT handle runs its launched loop while a preconditioner is set
 * (cgamd_dist_loop_launches says so: the slab loop has no preconditioned form); on a CGAMD_DIST_SINGLE_REDUCTION handle the three
 * calls return CGAMD_ERR_STATE (that loop has no PCG form).
 *   cgamd_dist_set_preconditioner        z = m_local .* r: n_local values of the handle's type, device pointer (copied); NULL removes any
 *                                        preconditioner -- the handle then returns the bits of one that never had any.
 *   cgamd_dist_set_preconditioner_jacobi m[i] = 1 / A_local[i][i], built on the device from the rank's matrix (the diagonal of local
 *                                        row i is local column i).  CGAMD_ERR_INVALID names the smallest LOCAL row whose diagonal is
 *                                        zero, missing or not finite.
 *   cgamd_dist_set_preconditioner_line   M = the local entries at column - row in {-stride, 0, +stride} WITH column < n_local: halo
 *                                        columns (local indices n_local ... n_local + n_halo - 1) are never line neighbours, so lines
 *                                        end at the rank's row range (with z-slab partitions of an x-fastest grid only z-lines are
 *                                        cut).  Extracted, factored (no pivoting) and planned on the device as for
 *                                        cgamd_solver_set_preconditioner_line, errors with the same wording and the local row;
 *                                        stride in [1, n_local - 1]. */
int cgamd_dist_set_preconditioner(cgamd_dist *d, const void *m_local);
int cgamd_dist_set_preconditioner_jacobi(cgamd_dist *d);
int cgamd_dist_set_preconditioner_line(cgamd_dist *d, int stride);
/* Multigrid on the row-partitioned handle: block-Jacobi over the ranks with a LOCAL hierarchy.  M^-1 on a rank is one V-cycle
 * (cgamd_solver_set_preconditioner_multigrid / _amg: same algorithm, defaults with 0, argument checks, error wording and level naming)
 * of a hierarchy built from the rank's CUT MATRIX: its rows with every entry at a halo column (>= n_local) removed, stored order kept --
 * the rank's diagonal block of A, symmetric positive definite whenever A is; the rule of the line preconditioner ("halo columns are
 * never line neighbours") for a whole matrix.  The cut matrix is a second copy of the rank's columns and values kept by the handle
 * (nnz_local entries at most) and runs the as-passed SpMV, not the coded one.  Errors name the LOCAL row.
 *   _multigrid  (nx, ny, nz) is the rank's OWN box, x fastest: nx * ny * nz != n_local is CGAMD_ERR_INVALID.  The caller vouches
 *               that its row range is that box (z-slabs of whole planes are).
 *   _amg        aggregates matched from the cut matrix: any row range, one that falls mid-line included.
 * Contracts of the three entries above: collective in meaning and local in execution, in force from the next cgamd_dist_set_rhs, a
 * failed call leaves the handle as it was, cgamd_dist_set_preconditioner(d, NULL) removes the hierarchy, CGAMD_DIST_SINGLE_REDUCTION
 * gets CGAMD_ERR_STATE, a CGAMD_DIST_RESIDENT handle runs its launched loop meanwhile.  Every launched loop is served, captured or
 * not, and cgamd_dist_iterate_until (the r update guarded; the cycle and the r.z partials unguarded; communication unchanged).  An
 * iteration: [SpMV + halo] [all-reduce d.q, alpha] [r -= alpha q, r.r] [the cycle's chain of launches, z over q] [r.z] [all-reduce
 * of both, beta, x += alpha d, d = z + beta d]: cgamd_dist_loop_launches is the preconditioned loop's count plus one plus the
 * cycle's launches.  cgamd_dist_refresh_values refills the cut values and builds the hierarchy again (removed if that fails).
 * cgamd_dist_mg_levels / _mg_level / _mg_level_matrix: as the cgamd_solver_mg_* accessors, level 0 the cut matrix.
 * cgamd_dist_mg_apply: z = one V-cycle of r, n_local device values each; synchronises (development accessor, like the two before). */
int cgamd_dist_set_preconditioner_multigrid(cgamd_dist *d, int nx, int ny, int nz, int smooth_steps, double over_correction, int min_rows);
int cgamd_dist_set_preconditioner_amg(cgamd_dist *d, int passes, double strength, int smooth_steps, double over_correction, int min_rows);
int cgamd_dist_mg_levels(cgamd_dist *d);
int cgamd_dist_mg_level(cgamd_dist *d, int level, long long info[6]);
int cgamd_dist_mg_level_matrix(cgamd_dist *d, int level, int *ptr, int *cols, void *vals);
int cgamd_dist_mg_apply(cgamd_dist *d, const void *r_dev, void *z_dev);   /* n_local values each */
/* The rank's matrix values (always borrowed) were changed in place on the same pattern: as cgamd_solver_refresh_values(s, NULL, 0).
 * Same contract: change the values only between solves, call this on EVERY rank before the next cgamd_dist_set_rhs.  Rank-local (it
 * does not communicate; DistSolver.refresh_values all-gathers the status).  The value codes follow on every loop (RCCL, both
 * peer-to-peer forms, single-reduction, slab); a captured graph is dropped when the code array was replaced; a Jacobi, line
 * or multigrid preconditioner built from the matrix is built again, and removed if that fails.  cgamd_dist_last_refresh: as
 * cgamd_solver_last_refresh (the outcome may differ from rank to rank). */
int cgamd_dist_refresh_values(cgamd_dist *d);
int cgamd_dist_last_refresh(cgamd_dist *d);
/* Peer-to-peer backend (CGAMD_DIST_P2P): instead of RCCL, every rank owns an uncached IPC-shared mailbox
 * (16 KiB header + n_halo values) that its peers write over xGMI; all-reduces are sums in rank order of values
 * deposited in per-rank slots (bitwise identical on all ranks).  Sequence: mailbox_alloc on every rank -> gather
 * the 64-byte handles of all ranks (torch.distributed) -> dist_create(..., id128 = NULL, flags | CGAMD_DIST_P2P)
 * -> attach_p2p(handles[nranks*64], dst_offset[n_peers] = where my entries land in each peer's halo area). */
int cgamd_p2p_mailbox_alloc(cgamd_ctx *ctx, long long halo_values, int dtype, void **mailbox, void *handle64);
int cgamd_p2p_mailbox_free(cgamd_ctx *ctx, void *mailbox);
int cgamd_dist_attach_p2p(cgamd_dist *d, void *my_mailbox, const void *handles, const int *dst_offset);
int cgamd_dist_p2p_error(cgamd_dist *d);
/* CGAMD_DIST_RESIDENT on a peer-to-peer handle that has peers: the slab loop publishes d in two buffers of n_local + n_halo values
 * inside every rank's mailbox allocation, behind the halo area (mailbox = 16 KiB header | n_halo values | ds0 | ds1, each part
 * rounded up to 256 bytes), so the peers write their boundary entries into the tail directly.  Allocate the mailbox with
 * halo_values >= n_halo + 2 (n_local + n_halo) + 96 (cgamd_p2p_mailbox_alloc), attach, then call this with that halo_values and every
 * rank's n_local / n_halo (all-gathered by the host).  OK whether or not the loop applies; cgamd_dist_loop_launches() == 0 tells. */
int cgamd_dist_enable_resident(cgamd_dist *d, long long mailbox_values, const int *rank_n_local, const int *rank_n_halo);
/* as cgamd_solver_index_codes, for this rank's local matrix (the halo columns of a slab partition sit at constant offsets) */
int cgamd_dist_index_codes(cgamd_dist *d);
/* stream operations per iteration of the loop this handle runs (kernel launches, plus RCCL calls with that backend); with a
 * preconditioner set, of the preconditioned loop (the same counts; two more where a stride-1 line sweep takes its long form; with multigrid
 * one more and the launches of the V-cycle) */
int cgamd_dist_loop_launches(cgamd_dist *d);
/* What the slab loop (CGAMD_DIST_RESIDENT, csrc/slab.hip) of this handle runs on; reads the plan, launches nothing, changes nothing.
 * info = {in use (0/1: as cgamd_dist_loop_launches() == 0), members G, rows of the largest member, 512-row steps of the largest member,
 * row unroll (5 / 7 / 8), register budget in steps (10 / 12), values from one-byte value codes (1) or streamed (0), uniform members
 * (1) or the unequal ones of a rank with peers (0)}; all zeros when the loop is not in use.  member_start receives the G + 1 member
 * starts (m * rows_m clipped to n_local when uniform; multiples of 1024, the last one rounded up, otherwise) when cap >= G + 1 and is left
 * alone otherwise.  Returns G + 1 (the count needed), 0 when the loop is not in use, negative on a null handle or null info. */
int cgamd_dist_slab_plan(cgamd_dist *d, int info[8], int *member_start, int cap);
/* number of ranks of the RCCL communicator behind this handle as RCCL itself reports it (ncclCommCount);
 * 0 when the handle has no communicator (peer-to-peer backend, or one rank without peers) */
int cgamd_dist_comm_ranks(cgamd_dist *d);

/* ---- Solution projection: start each solve from the span of earlier ones (csrc/projection.hip; Fischer, "Projection techniques
 * for iterative solution of Ax = b with successive right-hand sides", 1998).  A handle that serves a sequence of right-hand sides
 * keeps up to `capacity` vectors w_j per right-hand-side column, A-orthonormal in the handle's unconjugated inner product:
 * <w_i, A w_j> = delta_ij with <a, b> = sum a_i b_i.  Every column keeps a basis of its own (on a batched handle column r uses matrix r).
 * It only chooses x0, so it composes with every loop and every preconditioner of the handle.
 *   GUESS (cgamd_solver_set_rhs_projected): alpha_j = <w_j, b> for the held slots; x0 = sum_j alpha_j w_j, slots ascending from +0,
 *     one rounding per operation in the value type (x0 = 0 with no slot held); then cgamd_solver_set_rhs(s, b, x0), unchanged: the
 *     result is, bit for bit, what the caller gets by reading the guess (cgamd_solver_projection_state, which 1) and calling
 *     cgamd_solver_set_rhs with it.
 *   UPDATE (cgamd_solver_projection_update), from the x that cgamd_solver_get_x would return: e = x - x0 (with a full ring:
 *     e = (x - x0) + alpha_ret w_ret, see RING), q = A e (the handle's own SpMV), c_j = <w_j, q>; e' = e - sum_j c_j w_j, one classical Gram-Schmidt pass, slots ascending, all c_j from the same q;
 *     q' = A e', nu = <e', q'> (a second SpMV, not <e, q> - sum c_j^2, which cancels); s = sum alpha_j^2 + 2 sum alpha_j c_j + <e, q>
 *     over the slots that take part (<x, A x> in exact arithmetic; formed in the accumulation type).  A column's vector is accepted when nu is finite and
 *     |nu| > drop_tol^2 |s|, for the real types also nu > 0.  An accepted column stores w_new = e' * (1 / sqrt nu) -- the principal
 *     square root for the complex types, 1 / sqrt nu formed in the accumulation type and rounded once -- and a refused column stores
 *     a column of zeros, so that all columns keep one common slot count.  If every column is refused, nothing is retired and nothing
 *     is stored.
 *   RING: slots fill in order 0, 1, ...; with count == capacity the oldest slot is retired before the update -- its c_j is not formed
 *     and it takes no part in e' -- and w_new takes its place (dropping a member of an A-orthonormal set leaves the rest
 *     A-orthonormal: no restart).  What the retired vector carried of the guess stays in what is added: e = (x - x0) + alpha_ret w_ret,
 *     that is x minus the guess of the slots that stay.  (The oldest vector of a sequence of similar solutions is the direction they
 *     share -- every later one was orthogonalised against it -- so dropping it without this would leave a basis of differences: the
 *     first solve after the ring wraps then takes as many iterations as from zero.)
 *   Padding rows (cgamd_solver_ld) of every stored vector are 0.  The caller's arrays keep stride `size`.
 * Scalars: alpha_j and c_j are summed in double / complex double and rounded once to the value type, stored at [slot * nRHS + r];
 * nu, s and <e, q> stay in the accumulation type.
 * ORDER OF THE SUMS (fixed: two calls return the same bits).  <w_j, v> over `size` values with G = cgamd_projection_dots_grid(dtype,
 * size) work-groups of 256 threads and E = 16 / sizeof(value) values per 16-byte pack: thread t of work-group g starts from +0 and
 * adds the products (rounded in the value type, then widened) of packs g 256 + t + k G 256, k = 0, 1, ..., the E values of a pack in
 * order, then value E floor(size / E) + g 256 + t of the scalar tail; the 256 thread sums of a work-group are added by the wave tree
 * v[l] += v[l + off], off = 32 ... 1, and the four wave sums in order; the G work-group sums by one 1024-thread work-group: thread t
 * adds p[t], p[t + 1024], ..., then the wave tree and the 16 wave sums in order.  (With a pointer that is not 16-byte aligned, or
 * nRHS > 1 and ld or slot_pitch not whole packs, E = 1.)  <e, q> and nu: the order of cgamd_vdot's partials on the same G.
 * BYTES, V = sizeof(value), n = cgamd_solver_ld, m slots held (the basis is read once; v once per group of at most 8 slots):
 *   guess   (m + ceil(m / 8) + 1) n V nRHS          the dots pass m + ceil(m / 8), the combine pass m read + 1 written
 *   update  two SpMVs, then (3 + m + ceil(m / 8) + 4 + m + 2 + 2) n V nRHS: e = x - x0 (3), the dots pass (m + ceil(m / 8)), <e, q>
 *           and nu (2 + 2), the combine pass (m + 2), the store pass (2); with a full ring m - 1 for m in the dots and combine passes
 *           and 4 for e (it reads the retired vector)
 * cgamd_solver_projection_enable: capacity 1 ... 32 allocates capacity * nRHS * ld values plus one x0 block (CGAMD_ERR_ALLOC on
 *   failure, the handle unchanged) and starts with no slot held; capacity 0 disables the feature and frees the storage.  drop_tol >= 0
 *   and finite; 0 accepts every finite vector (nu > 0 for the real types).
 * cgamd_solver_projection_count: slots held, 0 ... capacity; 0 when disabled; negative on error.
 * cgamd_solver_projection_clear: count = 0, the storage is kept.
 * cgamd_solver_set_rhs_projected: CGAMD_ERR_STATE when the feature is not enabled.
 * cgamd_solver_projection_update: CGAMD_ERR_STATE unless the last right-hand side came through cgamd_solver_set_rhs_projected; may
 *   follow cgamd_solver_iterate, _iterate_until (frozen columns: their stopping iterate) and _iterate_tol.  x stays readable with
 *   cgamd_solver_get_x.  Afterwards the next call must be a set_rhs of either kind: the update uses the handle's q and d storage, so
 *   cgamd_solver_iterate, _iterate_until, _iterate_tol, _iterate_timed and _replace_residual return CGAMD_ERR_STATE, and so does a
 *   second update without a new solve.  added: nRHS ints (1 = the column's vector was accepted), may be NULL.  Synchronises once, to
 *   read the flags; nothing else crosses to the host.
 * cgamd_solver_refresh_values and cgamd_solver_reload_matrix clear the basis (the vectors were orthonormal for the old matrix);
 * changing or removing a preconditioner does not.
 * Served: every handle with RHS-major vectors (cgamd_solver_layout() == 0), all four value types, any nRHS, batched handles, every
 * preconditioner and loop, CGAMD_NO_GRAPH, CGAMD_UNFUSED, CGAMD_MATRIX_ON_DEVICE.  CGAMD_ERR_STATE, the handle untouched: row-major
 * layout; CGAMD_HERMITIAN on a complex type (the conjugated form is a later change).  CGAMD_ERR_INVALID: NULL handle, capacity
 * outside 0 ... 32, drop_tol negative or not finite, any of these calls while the stream is being captured. */
int cgamd_solver_projection_enable(cgamd_solver *s, int capacity, double drop_tol);
int cgamd_solver_projection_count(cgamd_solver *s);
int cgamd_solver_projection_clear(cgamd_solver *s);
int cgamd_solver_set_rhs_projected(cgamd_solver *s, const void *b, int on_device);
int cgamd_solver_projection_update(cgamd_solver *s, int *added /* nRHS ints, may be NULL */);
/* Development entries (tests; same standing as cgamd_solver_step_state).  _projection_state waits for the handle's stream and copies
 * to the host -- which 0: slot vector `slot`, nRHS x size values at stride size; 1: the guess x0, likewise; 2: alpha of the last guess,
 * capacity x nRHS values at [slot * nRHS + r]; 3: c of the last update, likewise (slots that took no part hold what they held);
 * 4: nu [nRHS], then s [nRHS] of the last update, in the accumulation type.
 * cgamd_projection_dots / _combine: the two basis kernels on DEVICE arrays of the caller, enqueued on the ctx stream.  Slot j of
 * column r starts at W + j * slot_pitch + r * ld values, column r of v and y at r * ld; bit j of live_mask says that slot j takes
 * part.  _dots: out[j * nRHS + r] = <w_j, v_r> for the live slots (the entry of a masked slot is untouched).  _combine:
 * y = v + sign * sum_j c_j w_j over the live slots, ascending, c at [j * nRHS + r], sign +1 or -1, v == NULL: y starts from +0; one
 * multiplication and one addition (subtraction) per slot per element; y may be v.  cgamd_projection_dots_grid: G above. */
int cgamd_solver_projection_state(cgamd_solver *s, int which, int slot, void *out_host);
int cgamd_projection_dots(cgamd_ctx *ctx, int dtype, int size, long long ld, int slots, unsigned live_mask,
                          const void *W, long long slot_pitch, const void *v, int nRHS, void *out /* device */);
int cgamd_projection_combine(cgamd_ctx *ctx, int dtype, int size, long long ld, int slots, unsigned live_mask,
                             const void *W, long long slot_pitch, const void *v, const void *c, int sign, void *y, int nRHS);
int cgamd_projection_dots_grid(int dtype, int size);

/* ---- Multi-shift CG: all (A + sigma_j I) x_j = b, j < S, on ONE SpMV per iteration (csrc/shifts.hip; Frommer and Maass, "Fast
 * CG-based methods for Tikhonov-Phillips regularization", 1999; Jegerlehner, "Krylov space solvers for shifted linear systems", 1996).
 * The Krylov spaces of the shifted systems are the seed's, and from x0 = 0 their residuals are multiples of the seed's residual,
 * r_k^j = zeta_k^j r_k.  So the handle runs its recurrence for A x = b unchanged -- the seed's x and history keep their bits -- and
 * every shift costs a few scalar operations and one pass over its own x_j and d_j.  The recurrence is algebraic in alpha_k and
 * beta_k: it serves the unconjugated recurrence on complex-symmetric matrices, with complex shifts.
 *   State per (shift j, right-hand side r): theta (= zeta_k / zeta_{k-1}), zeta, x_j, d_j.  At cgamd_solver_set_rhs: theta = zeta = 1,
 *   x_j = 0, d_j = r_0 = b; alpha_{-1} = 1, beta_{-1} = 0.  In iteration k, once alpha_k, beta_k and r_{k+1} exist:
 *     theta' = alpha_{k-1} / (alpha_k beta_{k-1} (1 - theta) + alpha_{k-1} (1 + sigma_j alpha_k))
 *     zeta'  = zeta theta' ;  alpha_j = alpha_k theta' ;  beta_j = beta_k theta' theta'
 *     x_j = x_j + alpha_j d_j ;  d_j = zeta' r_{k+1} + beta_j d_j
 *   This is the RATIO form: zeta underflows to 0 for a well-shifted system (sigma = 6 on a 200 x 200 Laplacian: exactly 0 after 900
 *   iterations), where the three-zeta form of the literature divides 0 / 0; here zeta = 0 only switches the r term off.
 *   Scalars: theta, zeta and the products in double / complex double (complex division by Smith's algorithm), from alpha_k and beta_k
 *   as the loop stores them in the value type; alpha_j, beta_j and zeta' are each rounded once to the value type.  Vectors: in the
 *   value type, one rounding per operation, x_j = x_j + (alpha_j * d_j), d_j = (zeta' * r) + (beta_j * d_j).
 *   LOOP: from set_rhs on, a handle with shifts in force runs the three / four-launch loop cgamd_solver_iterate_until runs (d in one
 *   buffer, x updated in every iteration; no two-launch, resident or deferred-x loop -- their bits are the same), and behind its d
 *   step the shift scalar step and ONE vector launch for all shifts: cgamd_solver_loop_launches() is that loop's count plus 2,
 *   whatever nShifts.  Captured graphs and CGAMD_NO_GRAPH give the same bits.
 *   cgamd_solver_iterate_until is served: the stop rule is unchanged (the SEED's delta_k per right-hand side), and a frozen
 *   right-hand side keeps, for every shift, the bits of cgamd_solver_iterate(its_r).  For positive shifts of a positive-definite
 *   matrix |zeta| <= 1 and the shifted systems have converged whenever the seed has; for other shifts read the shift history.
 * cgamd_solver_set_shifts: sigma = nShifts values of the handle's type in HOST memory, shared by all right-hand sides; nShifts
 *   1 ... 16; sigma == NULL or nShifts == 0 removes the shifts, and the handle then returns the bits of one that never had any.  Takes
 *   effect at the next cgamd_solver_set_rhs (which the next solve must start with).  Allocates 2 nShifts nRHS ld values
 *   (ld = cgamd_solver_ld), freed on removal and destroy.  A failed call leaves the handle unchanged.
 * cgamd_solver_shifts: shifts in force, 0 = none, negative on error.
 * cgamd_solver_get_x_shifted: x_j like cgamd_solver_get_x, nRHS x size values at the caller's stride `size`.
 * cgamd_solver_shift_history: entry k = zeta_k^j of every (j, r) in the value type, layout [k][j][r], k = 0 ... iterations done, row 0
 *   all ones; synchronises and returns the entries written (negative on error).  The residual of shifted system j is zeta_k^j r_k, so
 *   its delta_k^j = (zeta_k^j)^2 delta_k with delta_k of cgamd_solver_history -- unconjugated, like it.  A right-hand side frozen by
 *   cgamd_solver_iterate_until repeats its last entry.
 * Contract.  Served: single-system handles with RHS-major vectors, all four value types, any nRHS, CGAMD_NO_GRAPH,
 *   CGAMD_MATRIX_ON_DEVICE, CGAMD_SPLIT_LONG_ROWS, every SpMV form.  cgamd_solver_refresh_values and cgamd_solver_reload_matrix keep
 *   the shifts.  cgamd_solver_set_shifts returns CGAMD_ERR_STATE, the handle untouched, on batched handles, CGAMD_HERMITIAN on a complex
 *   type, CGAMD_UNFUSED, the row-major layout, and with a preconditioner in force (a preconditioned operator is not a shift of
 *   anything); CGAMD_ERR_INVALID for nShifts outside 0 ... 16 or a sigma that is not finite.  With shifts in force: CGAMD_ERR_STATE from
 *   every cgamd_solver_set_preconditioner* entry (except removal with NULL), cgamd_solver_iterate_tol, cgamd_solver_replace_residual and
 *   cgamd_solver_set_rhs_projected; CGAMD_ERR_INVALID from cgamd_solver_set_rhs with x0 != NULL.
 * Byte models: cgamd_solver_iter_bytes and cgamd_solver_iter_moved_bytes grow by (4 nShifts + 1) size V nRHS, V = sizeof(value): r
 *   read once for all shifts, x_j and d_j of every shift read and written (on top of the ten vector passes of the loop such a handle
 *   runs: x is updated in every iteration). */
int cgamd_solver_set_shifts(cgamd_solver *s, const void *sigma, int nShifts);
int cgamd_solver_shifts(cgamd_solver *s);
int cgamd_solver_get_x_shifted(cgamd_solver *s, int j, void *x, int on_device);
int cgamd_solver_shift_history(cgamd_solver *s, void *out, int max_entries);
/* Development entries (tests; same standing as cgamd_solver_step_state).  _shift_scalars waits for the handle's stream and copies the
 * last iteration's scalars to the host, nShifts x nRHS values at [j * nRHS + r] -- which 0: theta, 1: zeta, in double / complex
 * double; 2: alpha_j, 3: beta_j, in the value type.
 * cgamd_shift_update: the vector kernel alone on DEVICE arrays of the caller, enqueued on the ctx stream: r holds nRHS vectors at
 * stride ld, xs and ds nShifts x nRHS vectors, (j, r) at (j * nRHS + r) * ld; alpha_s, beta_s, zeta_s nShifts x nRHS values at
 * [j * nRHS + r].  xs_j = xs_j + alpha_j ds_j ; ds_j = zeta_j r + beta_j ds_j on the first `size` values of every vector; the rows
 * between size and ld are neither read nor written.  16-byte packs when r, xs, ds are 16-byte aligned and ld is whole packs, else
 * value by value: the same bits. */
int cgamd_solver_shift_scalars(cgamd_solver *s, int which, void *out_host);
int cgamd_shift_update(cgamd_ctx *ctx, int dtype, int size, long long ld, int nRHS, int nShifts, const void *r, void *xs, void *ds,
                       const void *alpha_s, const void *beta_s, const void *zeta_s);

/* ---- Block CG: the s = nRHS right-hand sides of one real SPD matrix share one Krylov space (csrc/block_cg.hip; O'Leary, "The block
 * conjugate gradient algorithm and related methods", 1980, in the residual-orthonormalised form of Dubrulle, "Retooling the method of
 * block conjugate gradients", 2001, "BCGrQ").  Every column searches the sum of all s Krylov spaces, so the block needs fewer
 * iterations than any single solve (5-point Laplacians, independent random right-hand sides: two to three times fewer at s = 16).  The
 * textbook recurrence is not built: its Gram matrices lose rank as the residuals shrink; here the residual block is kept as
 * R = Q xi with Q orthonormal, and the matrices factored stay well conditioned (pivot ratios of 0.4 and above on those systems).
 *   The handle's own vectors carry the block: x = X, r = Q, d = P, q = A P.  No n-sized buffer is allocated.
 *   At cgamd_solver_set_rhs: R0 = B - A X0 as ever; C = R0^T R0 = L L^T; xi = L^T; Q = R0 xi^-1; P = Q; history row 0 is
 *   delta_0[j] = |xi e_j|^2.  Iteration k, SIX launches whatever s, a linear chain:
 *     1  A P                                  the handle's multi-RHS SpMV in whatever form it has, its fused dot unused
 *     2  G = P^T (A P)                        per-work-group partials of the s (s + 1) / 2 distinct entries
 *     3  G = L L^T, alpha = G^-1, M = alpha xi        one work-group, in double, the partials summed in fixed order
 *     4  X += P M ; W = Q - (A P) alpha over Q        and the partials of W^T W; P, AP, X, Q read once, X and Q written once
 *     5  W^T W = L L^T, tau = L^T, tau^-1, xi <- tau xi, delta_k[j] = |xi e_j|^2 into the history; the stop word and the breakdown record
 *     6  Q <- W tau^-1 ; P <- Q + P tau^T      both in place
 *   Small matrices in double, left-looking Cholesky by columns, every inner sum in index order; alpha, M, tau^-1 and tau are each rounded
 *   once to the value type.  Vectors in the value type, one rounding per operation (tests/block_ref.py restates every order).
 *   Captured graphs and CGAMD_NO_GRAPH give the same bits; iterate(a); iterate(b) gives the bits of iterate(a + b).
 *   BREAKDOWN: a pivot v of either Cholesky counts as rank-deficient when not v > s eps_value max_j C_jj, C the matrix factored,
 *   eps_value = 2^-23 (float) or 2^-52 (double) -- a condition, not a tuned number: exact or linearly dependent columns give pivot
 *   ratios v / max_j C_jj of 5e-16 and below at set_rhs, healthy runs 0.4 and above.  The small step records which factorisation
 *   failed and the iteration, and freezes the loop: every later launch of the chain leaves at once and writes nothing.  X stays the
 *   last complete iterate: a failed G freezes before step 4, a failed W^T W after X is updated.  NaN freezes the same way.
 * cgamd_solver_set_block: on != 0 turns block CG on, on == 0 off.  Takes effect at the next cgamd_solver_set_rhs (x0 is allowed), which
 *   the next solve must start with; on = 0 returns the handle to the bits of one that never had it.  Returns CGAMD_ERR_STATE, the handle
 *   untouched, on complex types (the unconjugated block recurrence diverged on complex symmetric operators; the Hermitian block form
 *   is a later piece of work), batched handles, CGAMD_UNFUSED, the row-major layout, nRHS outside 2 ... 16, a preconditioner in force,
 *   shifts in force.  With block CG on: CGAMD_ERR_STATE from every cgamd_solver_set_preconditioner* entry (except removal with NULL),
 *   cgamd_solver_set_shifts, cgamd_solver_iterate_tol, cgamd_solver_replace_residual and cgamd_mixed_solve.
 *   cgamd_solver_set_rhs_projected stays served: projection only chooses x0.  cgamd_solver_refresh_values and
 *   cgamd_solver_reload_matrix keep the setting.
 * cgamd_solver_iterate(k) runs k block iterations.  cgamd_solver_iterate_until stops ALL columns in the first iteration in which
 *   every column satisfies its own tolerance -- the test of the plain loop, sqrt|delta_k[j]| >= tol[j] evaluated in double, on the
 *   history entry -- so iterations_run[r] are all equal; a breakdown ends the call with the count reached.  The host reads one device
 *   word per chunk as before, and the result does not depend on checkEvery.  cgamd_solver_history, cgamd_solver_get_x and
 *   cgamd_solver_iterations_done behave as ever; after a breakdown inside cgamd_solver_iterate, cgamd_solver_block_status brings
 *   cgamd_solver_iterations_done to the count reached.
 * cgamd_solver_block_status: waits for the handle's stream; info[0] on or off, info[1] status (0 running or stopped, 1 G failed,
 *   2 W^T W failed -- at iteration 0: R0^T R0 in set_rhs --, 3 NaN), info[2] the iteration of the event, info[3] s;
 *   *min_pivot_ratio (may be NULL) the smallest v / max_j C_jj since set_rhs.
 * Byte models: cgamd_solver_iter_bytes and cgamd_solver_iter_moved_bytes count the block loop's 14 vector passes per right-hand side
 *   (SpMV 2, Gram 2, step 4: 6, step 6: 4) beside the matrix; cgamd_solver_loop_launches is 6. */
int cgamd_solver_set_block(cgamd_solver *s, int on);
int cgamd_solver_block_status(cgamd_solver *s, int *info, double *min_pivot_ratio);
/* Development entries (tests; same standing as cgamd_shift_update).  _block_state waits for the handle's stream and copies one s x s
 * matrix to the host in double, row-major -- which 0: xi, 1: G, 2: alpha, 3: tau, 4: W^T W as summed (after set_rhs: R0^T R0),
 * 5: tau^-1, 6: M = alpha xi.
 * The vector kernels alone on DEVICE arrays of the caller, enqueued on the ctx stream; blocks hold s vectors at stride ld, the rows
 * between size and ld are neither read nor written; s x s factors in the value type, row-major, in device memory.  One thread owns a
 * row, so there is one path whatever the alignment of ld.
 * cgamd_block_gram: partials[p * grid + g], p = j (j + 1) / 2 + i, of a_i . b_j for i <= j, in double, grid = cgamd_block_gram_grid(size)
 *   work-groups (negative on error).  cgamd_block_update_xw: x_j = (..(x_j + p_0 m_0j) + ..) + p_s-1 m_s-1,j ; q_j = (..(q_j - ap_0
 *   alpha_0j) - ..) - ap_s-1 alpha_s-1,j, and the Gram partials of the new q with itself.  cgamd_block_update_qp: q_j = (..(q_0 ti_0j +
 *   q_1 ti_1j) + ..) + q_j ti_jj ; p_j = (..(q_j + p_j tau_jj) + ..) + p_s-1 tau_j,s-1 in place (init != 0: p_j = q_j), tau_inv and tau
 *   upper triangular. */
int cgamd_solver_block_state(cgamd_solver *s, int which, void *out_host);
int cgamd_block_gram_grid(int size);
int cgamd_block_gram(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, const void *a, const void *b, void *partials);
int cgamd_block_update_xw(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, const void *p, const void *ap, void *x, void *q,
                          const void *m, const void *alpha, void *partials);
int cgamd_block_update_qp(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, void *q, void *p, const void *tau_inv, const void *tau,
                          int init);

/* ---- Preconditioned block CG: the shared Krylov space with an M in force (csrc/block_pcg.hip).  BCGrQ as above, carried in the M^-1
 * inner product: R = Q xi with Q^T M^-1 Q = I.  The vectors carry the block as there -- x = X, r = Q, d = P, q = A P -- and q's storage
 * also holds Z = M^-1 W, because A P is dead once W exists.  No n-sized buffer is added.  M is the preconditioner in force: diagonal,
 * line or multigrid / AMG, whatever built it; "M^-1" below is what the scalar PCG loop applies between r and z.
 *   At cgamd_solver_set_rhs: R0 = B - A X0 as ever; Z0 = M^-1 R0 into q; C = R0^T Z0 = L L^T; xi = L^T; Q = R0 xi^-1; P = Z0 xi^-1;
 *   history row 0 is delta_0[j] = (R0^T R0)_jj: the history holds r.r, as on every preconditioned handle.  Iteration k, a linear chain:
 *     1  A P                                  the handle's SpMV as it is
 *     2  G = P^T (A P)                        the Gram launch of block CG
 *     3  G = L L^T, alpha = G^-1, M = alpha xi        the G step of block CG
 *     4  X += P M ; W = Q - (A P) alpha over Q        and the partials of W^T W: the launch of block CG, unchanged
 *     5  Z = M^-1 W into q                    the V-cycle or the line sweeps; for a diagonal M NOTHING runs here
 *     6  the partials of C = W^T Z            the Gram launch on (W, Z); for a diagonal M the weighted Gram: W read once, m once, entry
 *                                             (i <= j) = w_i . (m w_j) with m w_j rounded once in the value type, no Z block written or read
 *     7  the W step: both partial sets summed; delta_k[j] = (xi e_j)^T (W^T W) (xi e_j) with the OLD xi (R_k+1 = W xi_k) into the
 *        history and through the stop test; C = L L^T, tau = L^T, tau^-1, xi <- tau xi; the breakdown record
 *     8  Q <- W tau^-1 ; P <- Z tau^-1 + P tau^T      both in place; z_k read from Z, or m_i w_k rounded once (diagonal M)
 *   SEVEN launches and those of step 5: cgamd_solver_loop_launches is 7 plus the launches of z = M^-1 w (0 for a diagonal M).
 *   Orders: those of block CG (partials, their sums, the Cholesky, L^-1, alpha, M, tau xi); delta_k[j]: t_i = sum_m<=j (W^T W)_im xi_mj
 *   for i <= j, then sum_i<=j xi_ij t_i, every sum from its first product on, ascending (at set_rhs the diagonal entry itself).  Small
 *   matrices in double, each rounded once to the value type; vectors in the value type, one rounding per operation
 *   (tests/block_pcg_ref.py restates every order).  Captured graphs and CGAMD_NO_GRAPH give the same bits; iterate(a); iterate(b)
 *   gives the bits of iterate(a + b).
 *   BREAKDOWN: the pivot rule of block CG, not v > s eps_value max_j C_jj, on G and on C = W^T Z (R0^T Z0 at set_rhs).  An M that is not
 *   positive definite on the block therefore freezes the loop with status 2, as a dependent column does.  The history row of the
 *   iteration is written before C is factored.  Under cgamd_solver_iterate_until the M^-1 launches run unguarded, as in the scalar
 *   multigrid loop: what they write is read by nothing that writes.
 * cgamd_solver_set_block_pcg: on != 0 turns the mode on, legal only WITH a preconditioner in force; on == 0 returns the handle to the
 *   bits of the scalar PCG handle it was.  Takes effect at the next cgamd_solver_set_rhs (x0 is allowed).  Returns CGAMD_ERR_STATE,
 *   the handle untouched, when no preconditioner is in force and on everything cgamd_solver_set_block refuses -- complex types,
 *   batched handles, CGAMD_UNFUSED, the row-major layout, nRHS outside 2 ... 16, shifts in force -- and on CGAMD_HERMITIAN.
 *   cgamd_solver_set_block and cgamd_solver_set_block_pcg exclude each other: each refuses a handle the other has turned on.  While on,
 *   CGAMD_ERR_STATE from the entries block CG refuses, and from EVERY cgamd_solver_set_preconditioner* entry, removal with NULL
 *   too, because M is part of the state.  cgamd_solver_set_rhs_projected stays served.  cgamd_solver_refresh_values and
 *   cgamd_solver_reload_matrix keep the setting and rebuild an M that was built from the matrix (where that rebuild fails and M is
 *   removed, the mode goes with it).
 * cgamd_solver_block_status serves both modes: info[0] is 2 for the preconditioned one; status 2 means the second factorisation
 *   failed, here W^T Z (R0^T Z0 at iteration 0).  cgamd_solver_block_state: which = 7 is W^T Z as summed; 4 stays W^T W.
 * Byte models, vector passes per right-hand side beside the matrix: SpMV 2, Gram 2, step 4: 6, then for a diagonal M the weighted
 *   Gram 1 and step 8: 4 (15, and m read twice); for a line or multigrid M Gram (W, Z) 2 and step 8: 5 (17, and the preconditioner's
 *   own bytes as the scalar loop's model prices them).
 * Development entries (same standing as cgamd_block_gram): cgamd_block_gram_weighted: partials of w_i . (m w_j), m: `size` values
 *   shared by all columns.  cgamd_block_update_qp_z: q_j = (..(w_0 ti_0j + w_1 ti_1j) + ..) + w_j ti_jj (w: q on entry) and y_j the same
 *   expression over z_k; p_j = (..(y_j + p_j tau_jj) + ..) + p_s-1 tau_j,s-1 (init != 0: p_j = y_j); exactly one of z (the block) and m
 *   (z_k = m_i w_k rounded once) is non-NULL. */
int cgamd_solver_set_block_pcg(cgamd_solver *s, int on);
int cgamd_block_gram_weighted(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, const void *w, const void *m, void *partials);
int cgamd_block_update_qp_z(cgamd_ctx *ctx, int dtype, int size, long long ld, int s, void *q, void *p, const void *z, const void *m,
                            const void *tau_inv, const void *tau, int init);

#ifdef __cplusplus
}
#endif
#endif /* CGAMD_H */
