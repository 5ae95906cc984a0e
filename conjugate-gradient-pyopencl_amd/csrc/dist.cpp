// Row-partitioned multi-GPU CG: one process per GPU, RCCL over xGMI.
//
// The reference has no row partitioning (its multi-GPU mode replicates the matrix and splits the RHS
// columns over devices with zero communication: p_h-PY_C-CL-multi-GPU.py:2123-2181, cl.py:203-360);
// BASELINE.json's north star asks for the matrix to be row-partitioned, so this file is new design:
//
//   rank g owns a contiguous row block; its CSR slice has columns renumbered to
//   [0,n_local) = own entries of d, [n_local, n_local+n_halo) = entries owned by other ranks.
//   d lives in one extended buffer d_ext[n_local + n_halo]; the SpMV gathers from it directly.
//   Per iteration:  pack boundary entries -> grouped ncclSend/ncclRecv with the neighbours (the
//   "boundary all-gather" restricted to the entries actually referenced) -> SpMV fused with the local
//   d.q partials -> ncclAllReduce(1 scalar) -> x/r update fused with local r.r partials ->
//   ncclAllReduce(1 scalar) -> d update.  alpha/beta are computed redundantly on every rank from the
//   reduced scalars; there is no host synchronisation anywhere in the loop.
//
// RCCL is bound at run time with dlopen so that the single-GPU library has no link-time dependency
// on it (torch ships its own librccl.so.1; whichever copy is already in the process is reused).
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "cgamd_internal.h"
#include "launch_util.h"
#include "precond_state.h"

using namespace cgamd;

namespace {
struct Rccl {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
std::once_flag g_rccl_once;
std::string g_rccl_err;

void load_rccl() {
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) {
        g_rccl.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (g_rccl.handle) break;
    }
    if (!g_rccl.handle) { g_rccl_err = std::string("dlopen(librccl.so.1): ") + dlerror(); return; }
#define BIND(field, sym)                                                             \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(g_rccl.handle, sym)); \
    if (!g_rccl.field) { g_rccl_err = std::string("dlsym(") + sym + ") failed"; return; }
    BIND(GetUniqueId, "ncclGetUniqueId")
    BIND(CommInitRank, "ncclCommInitRank")
    BIND(CommDestroy, "ncclCommDestroy")
    BIND(CommCount, "ncclCommCount")
    BIND(AllReduce, "ncclAllReduce")
    BIND(Send, "ncclSend")
    BIND(Recv, "ncclRecv")
    BIND(GroupStart, "ncclGroupStart")
    BIND(GroupEnd, "ncclGroupEnd")
    BIND(GetErrorString, "ncclGetErrorString")
#undef BIND
}
int need_rccl() {
    std::call_once(g_rccl_once, load_rccl);
    if (!g_rccl_err.empty()) return fail(CGAMD_ERR_COMM, g_rccl_err);
    return CGAMD_OK;
}
#define CG_NCCL(expr)                                                                                     \
    do {                                                                                                  \
        ncclResult_t r__ = (expr);                                                                        \
        if (r__ != ncclSuccess)                                                                           \
            return fail(CGAMD_ERR_COMM, std::string(#expr) + ": " + g_rccl.GetErrorString(r__));          \
    } while (0)
}  // namespace

struct cgamd_dist {
    Tuning tune;            // configuration this handle was created under (installed per call: TuneScope)
    cgamd_ctx *ctx = nullptr;
    int dtype = 0, rank = 0, nranks = 1, n_local = 0, n_halo = 0, flags = 0;
    long long nnz = 0;
    const void *vals = nullptr;
    const int *ptr = nullptr, *cols = nullptr;
    SpmvPlan plan;
    int vgrid = 1;
    void *x = nullptr, *r = nullptr, *q = nullptr, *d_ext = nullptr, *b = nullptr;
    std::vector<int> peer, send_count, recv_count, send_off, recv_off;
    int total_send = 0;
    const int *send_index = nullptr;
    void *sendbuf = nullptr;
    void *part_dq = nullptr, *part_rr = nullptr;
    void *red = nullptr;  // 2 accumulator scalars: [0] = d.q, [1] = r.r
    CgScalars sc;
    ncclComm_t comm = nullptr;
    bool rhs_set = false;
    int iters = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    bool graph_failed = false;
    // peer-to-peer backend (no RCCL): uncached IPC mailboxes written directly by the peers over xGMI
    bool p2p = false, p2p_attached = false;
    char *my_mailbox = nullptr;
    std::vector<void *> opened;            // mappings to close
    char **mailbox_dev = nullptr;          // device array [nranks]
    int *plan_dev = nullptr;               // device: peer_rank, send_off, send_count, dst_off, recv_off, recv_count
    unsigned long long *epochs = nullptr;  // device: [0] exchange, [1] reduce slot 0, [2] reduce slot 1
    P2pExchange xch;
    // overlap of the boundary exchange with the SpMV of the interior row blocks
    bool overlap = false;
    int *interior_list = nullptr, *boundary_list = nullptr;   // device
    int n_interior = 0, n_boundary = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // four-launch peer-to-peer iteration: per-row-block flag "references a halo column" and the row block the SpMV
    // launch starts from (the leading boundary blocks of a slab partition are visited last)
    bool direct = false;
    int *halo_flag = nullptr;
    int rotate = 0;
    // one-byte column codes of the local matrix (build_index_codes; halo columns of a slab partition sit at constant offsets too)
    unsigned char *codes = nullptr;
    int *dict = nullptr;
    int n_offsets = 0;
    unsigned char *vcodes = nullptr;    // one-byte value codes on top (build_value_codes), with their dictionary
    void *vdict = nullptr;
    int n_values = 0;
    // single-reduction loop (CGAMD_DIST_SINGLE_REDUCTION, cg1.hip).  Roles of the buffers there: d_ext = r (the residual is what the
    // SpMV gathers, so it carries the halo), r = p, q = w = A r, s2 = s = A p
    bool cg1 = false;
    void *s2 = nullptr, *cg1_state = nullptr, *part_cg1 = nullptr;
    // slab loop (CGAMD_DIST_RESIDENT, slab.hip): every iteration of an iterate() call in one launch, vectors in registers
    SlabPlan slab, slab_plan_;         // slab: in use (ok); slab_plan_: what create found, waiting for its buffers (peer-to-peer handles)
    int *slab_map = nullptr;            // member starts [G + 1] and granule owners of a non-uniform slab partition
    std::vector<int> slab_mstart;       // host copy of those member starts (cgamd_dist_slab_plan); empty = uniform members
    void *slab_sync = nullptr, *ds_own[2] = {nullptr, nullptr};     // ds_own: plain buffers of a handle without peers
    void *ds[2] = {nullptr, nullptr};  // where the slab loop publishes d: ds_own, or inside the rank's mailbox allocation
    void **push_dst_dev = nullptr;     // device [2][n_peers]
    std::vector<char *> mailbox_host;  // mapped mailbox bases (host copy of mailbox_dev)
    std::vector<int> xch_dst_off;      // where my entries land in each peer's halo numbering
    SlabComm slab_comm;
    int n_cus = 0;
    // the preconditioner in force (precond_state.h; cgamd_dist_set_preconditioner*): pre.kind decides the loop -- a diagonal, lines
    // (factors cut at the rank's row range) or multigrid (below) -- and pre.built what cgamd_dist_refresh_values builds again.
    // z = M^-1 r lives in q's storage; the partials of r.z and r.r are [2][P] accumulators: part_pcg with P = vgrid for the diagonal
    // and multigrid loops (allocated at the first such M and kept), pre.tri_part with P = the sweeps' grid for the lines (pcg_prz,
    // pcg_prr, pcg_P); pre.rho2 = parity buffer of rho = r.z (delta holds rho for cg_alpha, history keeps r.r)
    Precond pre;
    void *part_pcg = nullptr;
    int last_refresh = 0;   // what the last cgamd_dist_refresh_values did (cgamd_dist_last_refresh)
    // multigrid (cgamd_dist_set_preconditioner_multigrid / _amg): one V-cycle of a hierarchy built from the CUT matrix,
    // the rank's rows without their halo columns (dist_cut.hip) -- a second, uncoded copy of the rank's columns and values with
    // n_pad - n_local empty rows behind them (n_pad: n_local rounded up to whole 16-byte packs, the rows mg_build's level 0 works
    // on).  r and q are allocated to n_pad values, so the cycle runs on them in place; the padding of r is zeroed at set_rhs.
    // The cut matrix lives and dies with pre.mg (pre_replaced)
    struct CutMatrix {
        int *ptr = nullptr, *cols = nullptr;
        void *vals = nullptr;
        long long nnz = 0;
        SpmvPlan plan;
    } cut;
    int n_pad = 0;
    // cgamd_dist_iterate_until: the stop (StopRun with one right-hand side: allocated at the first call, armed once per set_rhs).
    // until_stopped: the handle is frozen until the next set_rhs
    StopRun stop;
    bool until_stopped = false;
};

static void free_cut(cgamd_dist::CutMatrix *c) {
    for (void *p : {(void *)c->ptr, (void *)c->cols, c->vals})
        if (p) (void)hipFree(p);
    *c = cgamd_dist::CutMatrix();
}

static ncclDataType_t elem_type(int dtype) { return (dtype == CGAMD_F32 || dtype == CGAMD_C64) ? ncclFloat : ncclDouble; }
static size_t elem_mult(int dtype) { return (dtype == CGAMD_C64 || dtype == CGAMD_C128) ? 2 : 1; }

// boundary exchange of `v_ext[0:n_local]` into `v_ext[n_local:]` of the neighbours
static int exchange(cgamd_dist *d, void *v_ext, hipStream_t st) {
    if (d->peer.empty()) return CGAMD_OK;
    if (d->p2p) {
        if (!d->p2p_attached) return fail(CGAMD_ERR_STATE, "p2p backend: call cgamd_dist_attach_p2p first");
        return launch_p2p_exchange(d->dtype, d->xch, v_ext, st);
    }
    const size_t vs = dtype_size(d->dtype), em = elem_mult(d->dtype);
    if (int rc = launch_pack(d->dtype, d->total_send, d->send_index, v_ext, d->sendbuf, st)) return rc;
    CG_NCCL(g_rccl.GroupStart());
    for (size_t p = 0; p < d->peer.size(); ++p) {
        if (d->send_count[p])
            CG_NCCL(g_rccl.Send((const char *)d->sendbuf + (size_t)d->send_off[p] * vs, (size_t)d->send_count[p] * em,
                                elem_type(d->dtype), d->peer[p], d->comm, st));
        if (d->recv_count[p])
            CG_NCCL(g_rccl.Recv((char *)v_ext + ((size_t)d->n_local + d->recv_off[p]) * vs, (size_t)d->recv_count[p] * em,
                                elem_type(d->dtype), d->peer[p], d->comm, st));
    }
    CG_NCCL(g_rccl.GroupEnd());
    return CGAMD_OK;
}

static int allreduce_scalar(cgamd_dist *d, void *acc, hipStream_t st, int count = 1) {
    if (!d->comm) return CGAMD_OK;
    CG_NCCL(g_rccl.AllReduce(acc, acc, (size_t)count * acc_size(d->dtype) / 8, ncclDouble, ncclSum, d->comm, st));
    return CGAMD_OK;
}

// partials -> global sum -> the scalar step consuming it (mode 1 delta0, 2 alpha, 3 beta).  RCCL: local reduce,
// ncclAllReduce, scalar kernel (3 launches); peer-to-peer: one launch does all three.
// g (cgamd_dist_iterate_until): the guarded scalar step; the local reduce, the RCCL call and the mailbox round are the same either way
static int reduce_all(cgamd_dist *d, const void *partials, int count, int which, int mode, hipStream_t st, const CgStop *g = nullptr) {
    if (d->p2p) {
        if (!d->p2p_attached) return fail(CGAMD_ERR_STATE, "p2p backend: call cgamd_dist_attach_p2p first");
        return launch_p2p_allreduce(d->dtype, mode, partials, count, d->mailbox_dev, d->rank, d->nranks, which,
                                    d->epochs + 1 + which, d->sc, st, nullptr, nullptr, g);
    }
    void *out = (char *)d->red + 16 * which;
    if (int rc = launch_reduce_to_acc(d->dtype, partials, count, 1, out, st)) return rc;
    if (int rc = allreduce_scalar(d, out, st)) return rc;
    if (mode == 1) return launch_cg_delta0(d->dtype, out, 1, 1, d->sc, st);
    if (mode == 2) return launch_cg_alpha(d->dtype, out, 1, 1, d->sc, st, g);
    return launch_cg_beta(d->dtype, out, 1, 1, d->sc, st, g);
}

// ---- single-reduction loop (cg1.hip): [exchange of r] -> w = A r (+ r.w, r.r partials) -> ONE global sum -> alpha, beta and the
// four vector updates in one launch.  Peer-to-peer: two launches (the exchange rides in the SpMV launch, the sum in the update
// launch's prologue); RCCL: pack, send/recv, SpMV, local reduce, ncclAllReduce of two scalars, update (6 instead of 11 operations)
static Cg1Update cg1_update_args(cgamd_dist *d, bool p2p) {
    Cg1Update c;
    c.n = d->n_local; c.r = d->d_ext; c.p = d->r; c.s = d->s2; c.x = d->x; c.w = d->q;
    c.red = d->red; c.partials = d->part_cg1; c.P = d->plan.row_blocks;
    c.mailbox = p2p ? d->mailbox_dev : nullptr;
    c.rank = d->rank; c.nranks = d->nranks;
    c.slot_epoch = p2p ? d->epochs + 3 : nullptr;
    c.halo_epoch = p2p ? d->epochs : nullptr;
    c.state = d->cg1_state; c.sc = d->sc;
    return c;
}
static int enqueue_iteration_cg1(cgamd_dist *d, hipStream_t st) {
    const int dt = d->dtype, n = d->n_local;
    if (d->p2p && !d->p2p_attached) return fail(CGAMD_ERR_STATE, "p2p backend: call cgamd_dist_attach_p2p first");
    const bool p2p = d->p2p;
    int rc;
    if (!p2p && (rc = exchange(d, d->d_ext, st))) return rc;
    if ((rc = launch_spmv_cg1(dt, d->plan, n, d->nnz, d->vals, d->ptr, d->cols, d->d_ext, d->q, d->part_cg1, p2p ? d->halo_flag : nullptr,
                              p2p ? d->rotate : 0, p2p ? &d->xch : nullptr, d->sc.iter, p2p ? d->epochs + 3 : nullptr, st))) return rc;
    if (!p2p) {
        if ((rc = launch_reduce_to_acc(dt, d->part_cg1, d->plan.row_blocks, 2, d->red, st))) return rc;
        if ((rc = allreduce_scalar(d, d->red, st, 2))) return rc;
    }
    return launch_cg1_update(dt, cg1_update_args(d, p2p), st, d->plan.vec_nt);
}
// history[iterations done] = r.r of the current residual, in the partial-sum structure of the SpMV launch
static int enqueue_tail_cg1(cgamd_dist *d, hipStream_t st) {
    const int dt = d->dtype;
    const bool p2p = d->p2p;
    int rc;
    if ((rc = launch_cg1_rowblock_rr(dt, d->n_local, d->d_ext, (char *)d->part_cg1 + acc_size(dt) * (size_t)d->plan.row_blocks, st))) return rc;
    if (!p2p) {
        if ((rc = launch_reduce_to_acc(dt, d->part_cg1, d->plan.row_blocks, 2, d->red, st))) return rc;
        if ((rc = allreduce_scalar(d, d->red, st, 2))) return rc;
    }
    return launch_cg1_tail(dt, cg1_update_args(d, p2p), p2p ? d->epochs + 3 : nullptr, st);
}

// ---- preconditioned recurrence (cgamd_dist_set_preconditioner*): the SpMV (+ d.q) and the alpha step are the plain loop's, with
// delta = rho = r.z; then r -= alpha q and z = M^-1 r over q's storage with partials of r.z and r.r, ONE global round for the two
// sums, beta = rho / rho_old, x += alpha d, d = z + beta d.  M is rank-local (a diagonal, or lines cut at the row range): the
// sweep needs no communication.
static int pcg_P(const cgamd_dist *d) { return d->pre.kind == Precond::kTri ? d->pre.tri.grid : d->vgrid; }
static PcgPartials pcg_part(const cgamd_dist *d) {
    return pcg_partials(d->pre.kind == Precond::kTri ? d->pre.tri_part : d->part_pcg, d->dtype, pcg_P(d), 1);
}
static void *pcg_prz(const cgamd_dist *d) { return pcg_part(d).rz; }
static void *pcg_prr(const cgamd_dist *d) { return pcg_part(d).rr; }
// update = true: r -= alpha q first (z over q); false: set_rhs, z0 of r0 into `z`
static int pcg_sweep(cgamd_dist *d, bool update, void *z, hipStream_t st, const CgStop *g = nullptr) {
    const int dt = d->dtype, n = d->n_local;
    if (d->pre.kind == Precond::kMg) {
        // multigrid M, the single handle's branch on the distributed launches: r -= alpha q with the r.r partials (guarded), then
        // z = V-cycle(r) over q and the r.z partials -- both unguarded: z of a stopped handle is read by nothing that writes.  The
        // cycle is a linear chain of launches on st and works on n_pad rows of r and q (the padding of r is zero, of z comes out zero)
        int rc;
        if (update && (rc = launch_axpy_dot(dt, n, d->q, d->r, n, d->sc.alpha, 1, pcg_prr(d), pcg_P(d), st, d->plan.vec_nt, g))) return rc;
        if ((rc = mg_vcycle(d->pre.mg, d->r, d->q, st))) return rc;
        if (!update) {      // set_rhs: z0 goes to the local part of d_ext (whose halo part starts where the padding rows would lie)
            CG_HIP(hipMemcpyAsync(z, d->q, (size_t)n * dtype_size(dt), hipMemcpyDeviceToDevice, st));
            if ((rc = launch_dot_partials(dt, n, d->r, d->r, n, 1, pcg_prr(d), pcg_P(d), st))) return rc;
        }
        return launch_dot_partials(dt, n, d->r, z, n, 1, pcg_prz(d), pcg_P(d), st);
    }
    if (d->pre.kind == Precond::kDiag) {
        if (!update) return launch_pcg_axpy2_dot2(dt, true, n, z, d->x, d->q, d->r, d->pre.mdiag, n, nullptr, 1, pcg_prz(d), pcg_prr(d), pcg_P(d), st);
        return launch_pcg_jacobi_z(dt, n, d->q, d->r, d->pre.mdiag, d->sc.alpha, pcg_prz(d), pcg_prr(d), pcg_P(d), st, g);
    }
    const void *q = update ? d->q : nullptr, *alpha = update ? d->sc.alpha : nullptr;
    if (d->pre.tri.stride > 1) return launch_pcg_tri_strided(dt, d->pre.tri, update, q, d->r, z, n, alpha, 1, pcg_prz(d), pcg_prr(d), st, g);
    return launch_pcg_tri(dt, d->pre.tri, update, q, d->r, z, n, alpha, 1, pcg_prz(d), pcg_prr(d), st, g);
}
// {r.z, r.r} partials -> global sums -> the scalar step (mode 1 set_rhs, 3 beta).  RCCL: local reduce of two values, ONE ncclAllReduce
// of count 2, scalar kernel; peer-to-peer: one launch
static int pcg_reduce2(cgamd_dist *d, int mode, hipStream_t st, const CgStop *g = nullptr) {
    if (d->p2p) {
        if (!d->p2p_attached) return fail(CGAMD_ERR_STATE, "p2p backend: call cgamd_dist_attach_p2p first");
        return launch_pcg_allreduce2_p2p(d->dtype, mode, pcg_prz(d), pcg_prr(d), pcg_P(d), d->mailbox_dev, d->rank, d->nranks, d->epochs + 2,
                                         d->sc, d->pre.rho2, st, g);
    }
    if (int rc = launch_reduce_to_acc(d->dtype, pcg_prz(d), pcg_P(d), 2, d->red, st)) return rc;
    if (int rc = allreduce_scalar(d, d->red, st, 2)) return rc;
    return launch_pcg_scalars(d->dtype, mode, d->red, d->sc, d->pre.rho2, st, g);
}

// One iteration of the handle's launched loop and preconditioner.  g (cgamd_dist_iterate_until): the same launches with the guarded
// instantiation of every kernel that writes x, r, the local part of d_ext, a scalar, the history or the counter (stop_device.h, one
// right-hand side).  COMMUNICATION NEVER DEPENDS ON THE STOP: g reaches kernels only -- the halo push and wait (inside the SpMV
// launch, or the exchange launches / RCCL calls), every all-reduce round, every epoch bump and the overlap's fork / join run after
// the stop exactly as before it -- with d frozen the peers receive the same halo values and the sums repeat -- so no rank waits for
// one that left early, because none does.  The SpMV is the unguarded one: q of a frozen handle is recomputed and read by nothing.
static int enqueue_iteration(cgamd_dist *d, hipStream_t st, const CgStop *g = nullptr) {
    if (d->cg1) return enqueue_iteration_cg1(d, st);        // (no guarded form: cgamd_dist_iterate_until refuses such a handle)
    const int dt = d->dtype, n = d->n_local;
    const long long ldx = (long long)d->n_local + d->n_halo;
    int rc;
    if (d->direct && d->p2p_attached) {
        // peer-to-peer, four launches: [push | wait | SpMV | d.q], [all-reduce d.q, alpha], [r -= alpha q, r.r], [all-reduce r.r, beta, x += alpha d, aypx]
        if ((rc = launch_spmv_p2p(dt, d->plan, n, d->nnz, d->vals, d->ptr, d->cols, d->d_ext, d->q, d->part_dq, d->halo_flag,
                                  d->rotate, d->xch, st))) return rc;
        if ((rc = launch_p2p_allreduce(dt, 2, d->part_dq, d->plan.n_partials, d->mailbox_dev, d->rank, d->nranks, 0, d->epochs + 1,
                                       d->sc, st, d->epochs, d->epochs + 2, g))) return rc;
        if (d->pre.kind != Precond::kNone) {      // [r -= alpha q, z = M^-1 r, r.z, r.r], [all-reduce of both, beta, x += alpha d, d = z + beta d]
            if ((rc = pcg_sweep(d, true, d->q, st, g))) return rc;
            return launch_pcg_aypx_beta_p2p(dt, n, d->q, d->d_ext, d->x, pcg_prz(d), pcg_prr(d), pcg_P(d), d->mailbox_dev, d->rank, d->nranks,
                                            d->epochs + 2, d->sc, d->pre.rho2, st, d->plan.vec_nt, g);
        }
        if ((rc = launch_axpy_dot(dt, n, d->q, d->r, n, d->sc.alpha, 1, d->part_rr, d->vgrid, st, d->plan.vec_nt, g))) return rc;
        return launch_aypx_beta_p2p(dt, n, d->r, d->d_ext, d->x, d->part_rr, d->vgrid, d->mailbox_dev, d->rank, d->nranks, 1,
                                    d->epochs + 2, d->sc, st, d->plan.vec_nt, g);
    }
    if (d->overlap) {
        // fork: the exchange runs on the comm stream while the row blocks that reference no halo column are
        // multiplied; the boundary blocks follow once the halo has landed.  Both launches write disjoint
        // entries of q and of the d.q partials.
        CG_HIP(hipEventRecord(d->ev_fork, st));
        CG_HIP(hipStreamWaitEvent(d->comm_stream, d->ev_fork, 0));
        if ((rc = exchange(d, d->d_ext, d->comm_stream))) return rc;
        CG_HIP(hipEventRecord(d->ev_join, d->comm_stream));
        if ((rc = launch_spmv(dt, d->plan, n, d->nnz, d->vals, d->ptr, d->cols, d->d_ext, ldx, d->q, n, 1, d->d_ext, d->part_dq, st,
                              d->interior_list, d->n_interior))) return rc;
        CG_HIP(hipStreamWaitEvent(st, d->ev_join, 0));
        if ((rc = launch_spmv(dt, d->plan, n, d->nnz, d->vals, d->ptr, d->cols, d->d_ext, ldx, d->q, n, 1, d->d_ext, d->part_dq, st,
                              d->boundary_list, d->n_boundary))) return rc;
    } else {
        if ((rc = exchange(d, d->d_ext, st))) return rc;
        if ((rc = launch_spmv(dt, d->plan, n, d->nnz, d->vals, d->ptr, d->cols, d->d_ext, ldx, d->q, n, 1, d->d_ext, d->part_dq, st))) return rc;
    }
    if ((rc = reduce_all(d, d->part_dq, d->plan.n_partials, 0, 2, st, g))) return rc;
    if (d->pre.kind != Precond::kNone) {      // (guarded: x += alpha d rides in the last launch, which leaves on live[]: the stopping iteration still gets it)
        if ((rc = pcg_sweep(d, true, d->q, st, g))) return rc;
        if ((rc = pcg_reduce2(d, 3, st, g))) return rc;
        return launch_pcg_xd_update(dt, n, d->q, d->d_ext, d->x, d->sc, st, g);
    }
    // (guarded: x is updated BEFORE the deciding launch here, so the stopping iteration's x is in place when stop[] is written)
    if ((rc = launch_axpy2_dot(dt, n, d->d_ext, d->x, d->q, d->r, n, d->sc.alpha, 1, d->part_rr, d->vgrid, st, d->plan.vec_nt, g))) return rc;
    if ((rc = reduce_all(d, d->part_rr, d->vgrid, 1, 3, st, g))) return rc;
    return launch_aypx(dt, n, d->r, d->d_ext, n, d->sc.beta, 1, st, g);
}

// classify the row blocks once: boundary = references a halo column
// the one-byte value codes on top of the column codes, for the values now in d->vals (create, refresh_values): the handle has none
// when this is called.  Every copy of the two pointers the handle keeps follows: the SpMV plan, the slab plan in force, the pending one.
static bool value_codes_apply(const cgamd_dist *d) { return d->codes && d->tune.value_codes && d->plan.kind == 5 && d->dtype != CGAMD_C128; }
static void publish_value_codes(cgamd_dist *d) {
    d->plan.vcodes = d->vcodes; d->plan.vdict = d->vdict; d->plan.vcodes_for = d->vcodes ? d->vals : nullptr;
    d->slab.vcodes = d->vcodes; d->slab.vdict = d->vdict;
    d->slab_plan_.vcodes = d->vcodes; d->slab_plan_.vdict = d->vdict;
}
static void drop_value_codes(cgamd_dist *d) {
    if (d->vcodes) { (void)hipFree(d->vcodes); d->vcodes = nullptr; }
    if (d->vdict) { (void)hipFree(d->vdict); d->vdict = nullptr; }
    d->n_values = 0;
    publish_value_codes(d);
}
static int setup_value_codes(cgamd_dist *d) {
    if (!value_codes_apply(d)) return CGAMD_OK;
    const int rc = build_value_codes(d->dtype, d->nnz, d->vals, d->ctx->stream, &d->vcodes, &d->vdict, &d->n_values);
    publish_value_codes(d);
    return rc;
}

static int classify_row_blocks(cgamd_dist *d, std::vector<int> *interior, std::vector<int> *boundary) {
    const int nb = d->plan.row_blocks;
    int *flags_dev = nullptr;
    if (int rc = dmalloc((void **)&flags_dev, sizeof(int) * (size_t)nb, "halo flags")) return rc;
    int rc = launch_halo_flags(d->n_local, d->ptr, d->cols, d->n_local, nb, flags_dev, d->ctx->stream);
    std::vector<int> flags((size_t)nb);
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(flags.data(), flags_dev, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, d->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->ctx->stream);
    (void)hipFree(flags_dev);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CGAMD_ERR_HIP, std::string("halo flags: ") + hipGetErrorString(e));
    for (int rb = 0; rb < nb; ++rb) (flags[(size_t)rb] ? boundary : interior)->push_back(rb);
    return CGAMD_OK;
}

static int upload_ints(int **dev, const std::vector<int> &v, const char *what) {
    if (int rc = dmalloc((void **)dev, sizeof(int) * v.size(), what)) return rc;
    if (!v.empty()) CG_HIP(hipMemcpy(*dev, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice));
    return CGAMD_OK;
}

static int build_overlap_lists(cgamd_dist *d, const std::vector<int> &interior, const std::vector<int> &boundary) {
    const int nb = d->plan.row_blocks;
    if (nb < 16 || boundary.empty() || boundary.size() * 2 > (size_t)nb) return CGAMD_OK;   // nothing to hide it behind
    int rc;
    if ((rc = upload_ints(&d->interior_list, interior, "interior list"))) return rc;
    if ((rc = upload_ints(&d->boundary_list, boundary, "boundary list"))) return rc;
    d->n_interior = (int)interior.size();
    d->n_boundary = (int)boundary.size();
    CG_HIP(hipStreamCreateWithFlags(&d->comm_stream, hipStreamNonBlocking));
    CG_HIP(hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming));
    CG_HIP(hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming));
    d->overlap = true;
    return CGAMD_OK;
}

// four-launch peer-to-peer SpMV: flags per row block, visiting order rotated past the leading boundary blocks
static int build_direct_schedule(cgamd_dist *d, const std::vector<int> &boundary) {
    const int nb = d->plan.row_blocks;
    std::vector<int> flag((size_t)nb, 0);
    for (int rb : boundary) flag[(size_t)rb] = 1;
    int lead = 0;
    while (lead < nb && flag[(size_t)lead]) ++lead;
    d->rotate = lead < nb ? lead : 0;
    if (int rc = upload_ints(&d->halo_flag, flag, "halo flags")) return rc;
    d->direct = true;
    return CGAMD_OK;
}

static int ensure_history(cgamd_dist *d, int entries) {
    if (entries <= d->sc.history_cap) return CGAMD_OK;
    const int cap = std::max(entries, std::max(1024, d->sc.history_cap * 2));
    const size_t vs = dtype_size(d->dtype);
    void *nh = nullptr;
    if (int rc = dmalloc(&nh, (size_t)cap * vs, "history")) return rc;
    if (d->sc.history) {
        CG_HIP(hipStreamSynchronize(d->ctx->stream));
        CG_HIP(hipMemcpy(nh, d->sc.history, (size_t)d->sc.history_cap * vs, hipMemcpyDeviceToDevice));
        CG_HIP(hipFree(d->sc.history));
    }
    d->sc.history = nh;
    d->sc.history_cap = cap;
    if (d->gexec) { (void)hipGraphExecDestroy(d->gexec); d->gexec = nullptr; }
    if (d->graph) { (void)hipGraphDestroy(d->graph); d->graph = nullptr; }
    return CGAMD_OK;
}

extern "C" {

int cgamd_comm_unique_id(void *id128) {
    if (!id128) return fail(CGAMD_ERR_INVALID, "comm_unique_id: null buffer");
    if (int rc = need_rccl()) return rc;
    ncclUniqueId id;
    CG_NCCL(g_rccl.GetUniqueId(&id));
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id128, &id, 128);
    return CGAMD_OK;
}

int cgamd_dist_create(cgamd_ctx *ctx, const void *id128, int rank, int nranks, int dtype, int n_local, int n_halo,
                      long long nnz_local, const void *aValues, const int *aPointers, const int *aCols, int n_peers,
                      const int *peer_rank, const int *send_count, const int *recv_count, const int *send_index,
                      int flags, cgamd_dist **out) {
    if (!out) return fail(CGAMD_ERR_INVALID, "dist_create: out is NULL");
    *out = nullptr;
    if (flags & CGAMD_HERMITIAN)
        return fail(CGAMD_ERR_INVALID, "dist_create: CGAMD_HERMITIAN is a flag of the single-GPU handle (the row-partitioned loops run the unconjugated recurrence only)");
    if (!ctx) return fail(CGAMD_ERR_INVALID, "dist_create: ctx is NULL");
    if (dtype < 0 || dtype > 3) return fail(CGAMD_ERR_INVALID, "dist_create: bad dtype");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(CGAMD_ERR_INVALID, "dist_create: bad rank/nranks");
    if (n_local < 1 || n_halo < 0 || nnz_local < 0 || n_peers < 0) return fail(CGAMD_ERR_INVALID, "dist_create: bad sizes");
    if ((long long)n_local + n_halo > 2147483647LL || nnz_local > 2147483647LL - 8192)
        return fail(CGAMD_ERR_INVALID, "dist_create: local problem exceeds int32 indexing");
    if (!aValues || !aPointers || !aCols) return fail(CGAMD_ERR_INVALID, "dist_create: null matrix pointer");
    if (n_peers > 0 && (!peer_rank || !send_count || !recv_count)) return fail(CGAMD_ERR_INVALID, "dist_create: null plan arrays");
    if ((nranks > 1 || n_peers > 0) && !id128 && !(flags & CGAMD_DIST_P2P))
        return fail(CGAMD_ERR_INVALID, "dist_create: a communicator id (or CGAMD_DIST_P2P) is required when there are peers");
    CG_HIP(hipSetDevice(ctx->device));

    cgamd_dist *d = new cgamd_dist();
    d->tune = tune_snapshot();
    TuneScope ts(&d->tune);
    d->ctx = ctx; d->dtype = dtype; d->rank = rank; d->nranks = nranks; d->n_local = n_local; d->n_halo = n_halo;
    d->nnz = nnz_local; d->vals = aValues; d->ptr = aPointers; d->cols = aCols; d->flags = flags;
    d->p2p = (flags & CGAMD_DIST_P2P) != 0;
    d->cg1 = (flags & CGAMD_DIST_SINGLE_REDUCTION) != 0;
    d->plan = make_spmv_plan(n_local);
    d->vgrid = vec_grid(n_local, dtype);
    long long so = 0, ro = 0;
    for (int p = 0; p < n_peers; ++p) {
        if (peer_rank[p] < 0 || peer_rank[p] >= nranks || send_count[p] < 0 || recv_count[p] < 0) {
            delete d;
            return fail(CGAMD_ERR_INVALID, "dist_create: bad peer entry");
        }
        d->peer.push_back(peer_rank[p]);
        d->send_count.push_back(send_count[p]);
        d->recv_count.push_back(recv_count[p]);
        d->send_off.push_back((int)so);
        d->recv_off.push_back((int)ro);
        so += send_count[p];
        ro += recv_count[p];
    }
    if (ro != n_halo) { delete d; return fail(CGAMD_ERR_INVALID, "dist_create: sum(recv_count) != n_halo"); }
    if (so > 0 && !send_index) { delete d; return fail(CGAMD_ERR_INVALID, "dist_create: send_index is NULL"); }
    d->total_send = (int)so;
    d->send_index = send_index;

    const size_t vs = dtype_size(dtype);
    int rc = CGAMD_OK;
    if (!rc) rc = dmalloc(&d->x, (size_t)n_local * vs, "x");
    // (r and q to whole 16-byte packs: the multigrid cycle works on n_pad rows of them)
    {
        const int E = (int)(16 / vs);
        d->n_pad = n_local < 2147483647 - 8 ? (n_local + E - 1) / E * E : n_local;
    }
    if (!rc) rc = dmalloc(&d->r, (size_t)d->n_pad * vs, "r");
    if (!rc) rc = dmalloc(&d->q, (size_t)d->n_pad * vs, "q");
    if (!rc) rc = dmalloc(&d->b, (size_t)n_local * vs, "b");
    if (!rc) rc = dmalloc(&d->d_ext, ((size_t)n_local + n_halo) * vs, "d_ext");
    if (!rc) rc = dmalloc(&d->sendbuf, (size_t)so * vs, "sendbuf");
    if (!rc) rc = dmalloc(&d->part_dq, acc_size(dtype) * (size_t)std::max(d->plan.grid, d->plan.row_blocks), "partials_dq");
    if (!rc) rc = dmalloc(&d->part_rr, acc_size(dtype) * (size_t)d->vgrid, "partials_rr");
    if (!rc) rc = dmalloc(&d->red, 64, "red");
    if (!rc) rc = dmalloc(&d->sc.alpha, vs, "alpha");
    if (!rc) rc = dmalloc(&d->sc.beta, vs, "beta");
    if (!rc) rc = dmalloc(&d->sc.delta, vs, "delta");
    if (!rc) rc = dmalloc((void **)&d->sc.iter, 64, "iter");
    if (!rc) rc = ensure_history(d, 1024);
    if (!rc) rc = validate_csr_device(n_local, nnz_local, n_local + n_halo, d->ptr, d->cols, d->send_index, d->total_send, n_local, d->sc.iter,
                                      ctx->stream);
    if (!rc) rc = compute_spmv_plan(d->ptr, d->cols, n_local, d->sc.iter, ctx->stream, &d->plan);
    if (!rc) finalize_spmv_plan(&d->plan, dtype, 1, n_local, nnz_local, d->vals, d->cols);
    if (!rc && d->tune.index_codes && d->plan.kind == 5 && d->tune.index_codes_min_mb >= 0 &&
        (size_t)nnz_local * (dtype_size(dtype) + 4) > ((size_t)d->tune.index_codes_min_mb << 20)) {
        rc = build_index_codes(n_local, nnz_local, d->ptr, d->cols, ctx->stream, &d->codes, &d->dict, &d->n_offsets);
        if (!rc && d->codes) { d->plan.codes = d->codes; d->plan.dict = d->dict; d->plan.codes_for = d->cols; }
        if (!rc) rc = setup_value_codes(d);
    }
    if (!rc && d->cg1) {
        if (!cg1_supported(d->plan, d->vals, d->cols))
            rc = fail(CGAMD_ERR_INVALID, "dist_create: the single-reduction loop needs the row-block SpMV (16-byte aligned matrix arrays, rows "
                                         "whose 256-row slices fit LDS)");
        if (!rc) rc = dmalloc(&d->s2, (size_t)n_local * vs, "s");
        if (!rc) rc = dmalloc(&d->cg1_state, 64, "single-reduction state");
        if (!rc) rc = dmalloc(&d->part_cg1, acc_size(dtype) * 2 * (size_t)d->plan.row_blocks, "partials (r.w, r.r)");
    }
    if (!rc && (flags & CGAMD_DIST_RESIDENT) && !d->cg1) {
        if (hipDeviceGetAttribute(&d->n_cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess) d->n_cus = 0;
        if (d->tune.slab_cus > 0) d->n_cus = std::min(d->n_cus, d->tune.slab_cus);
        SlabPlan sp;
        if (slab_plan(dtype, n_local, d->n_cus, d->plan, d->codes != nullptr, &sp)) {
            sp.vcodes = d->vcodes; sp.vdict = d->vdict;      // (publish_value_codes keeps both copies current)
            rc = dmalloc(&d->slab_sync, sp.sync_bytes, "slab sync words");
            if (!rc && d->peer.empty() && nranks == 1) {     // nothing to exchange: plain buffers, usable at once
                for (int b = 0; b < 2 && !rc; ++b) rc = dmalloc(&d->ds_own[b], (size_t)n_local * vs, "published d");
                if (!rc) { d->ds[0] = d->ds_own[0]; d->ds[1] = d->ds_own[1]; d->slab = sp; }
            } else if (!rc && d->p2p) {
                d->slab_plan_ = sp;              // cgamd_dist_enable_resident finds the buffers inside the mailbox allocation
            }
        }
    }
    if (!rc && id128 && !d->p2p) {
        rc = need_rccl();
        if (!rc) {
            ncclUniqueId id;
            memcpy(&id, id128, 128);
            ncclResult_t r = g_rccl.CommInitRank(&d->comm, nranks, id, rank);
            if (r != ncclSuccess) rc = fail(CGAMD_ERR_COMM, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
        }
    }
    // hipGraph capture of the two-stream fork/join around RCCL send/recv crashed in the runtime (ROCm 7.0/7.2,
    // RCCL 2.26): with RCCL the graph mode therefore runs the exchange in line and the plain-launch mode overlaps
    // it; the peer-to-peer backend is pure kernels and overlaps in both modes.
    if (!rc && d->n_halo > 0 && d->plan.kind == 5) {
        std::vector<int> interior, boundary;
        rc = classify_row_blocks(d, &interior, &boundary);
        const bool staged = (flags & CGAMD_DIST_P2P_STAGED) != 0;
        if (!rc && d->p2p && (!staged || d->cg1)) rc = build_direct_schedule(d, boundary);
        if (!rc && !d->direct && !d->cg1 && !(flags & CGAMD_DIST_NO_OVERLAP) && ((d->comm && !(flags & CGAMD_DIST_GRAPH)) || d->p2p))
            rc = build_overlap_lists(d, interior, boundary);
    }
    if (rc) {
        std::string keep = cgamd_last_error();
        cgamd_dist_destroy(d);
        set_error(keep);
        return rc;
    }
    *out = d;
    return CGAMD_OK;
}

int cgamd_dist_destroy(cgamd_dist *d) {
    if (!d) return CGAMD_OK;
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    if (d->gexec) (void)hipGraphExecDestroy(d->gexec);
    if (d->graph) (void)hipGraphDestroy(d->graph);
    if (d->comm) (void)g_rccl.CommDestroy(d->comm);
    for (void *m : d->opened) (void)hipIpcCloseMemHandle(m);
    if (d->mailbox_dev) (void)hipFree(d->mailbox_dev);
    if (d->plan_dev) (void)hipFree(d->plan_dev);
    if (d->epochs) (void)hipFree(d->epochs);
    if (d->comm_stream) { (void)hipStreamSynchronize(d->comm_stream); (void)hipStreamDestroy(d->comm_stream); }
    if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
    if (d->ev_join) (void)hipEventDestroy(d->ev_join);
    stop_run_free(d->stop);
    if (d->interior_list) (void)hipFree(d->interior_list);
    if (d->boundary_list) (void)hipFree(d->boundary_list);
    if (d->halo_flag) (void)hipFree(d->halo_flag);
    if (d->codes) (void)hipFree(d->codes);
    if (d->vcodes) (void)hipFree(d->vcodes);
    if (d->vdict) (void)hipFree(d->vdict);
    if (d->dict) (void)hipFree(d->dict);
    free_cut(&d->cut);
    precond_drop(&d->pre);
    void *bufs[] = {d->x, d->r, d->q, d->b, d->d_ext, d->sendbuf, d->part_dq, d->part_rr, d->red, d->sc.alpha,
                    d->sc.beta, d->sc.delta, d->sc.history, d->sc.iter, d->s2, d->cg1_state, d->part_cg1, d->slab_sync, d->slab_map, d->ds_own[0], d->ds_own[1],
                    d->push_dst_dev, d->part_pcg, d->pre.rho2};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete d;
    return CGAMD_OK;
}

int cgamd_dist_set_rhs(cgamd_dist *d, const void *b_local, const void *x0_local) {
    if (!d || !b_local) return fail(CGAMD_ERR_INVALID, "dist_set_rhs: null argument");
    TuneScope ts(&d->tune);
    CG_HIP(hipSetDevice(d->ctx->device));
    hipStream_t st = d->ctx->stream;
    const size_t vs = dtype_size(d->dtype), vb = (size_t)d->n_local * vs;
    const long long ldx = (long long)d->n_local + d->n_halo;
    CG_HIP(hipMemcpyAsync(d->b, b_local, vb, hipMemcpyDeviceToDevice, st));
    if (x0_local) CG_HIP(hipMemcpyAsync(d->x, x0_local, vb, hipMemcpyDeviceToDevice, st));
    else CG_HIP(hipMemsetAsync(d->x, 0, vb, st));
    // r = b - A x0 (x0 exchanged through the extended buffer), d = r, delta0 = allreduce(r.r)
    CG_HIP(hipMemcpyAsync(d->d_ext, d->x, vb, hipMemcpyDeviceToDevice, st));
    int rc;
    if ((rc = exchange(d, d->d_ext, st))) return rc;
    if ((rc = launch_spmv(d->dtype, d->plan, d->n_local, d->nnz, d->vals, d->ptr, d->cols, d->d_ext, ldx, d->q, d->n_local, 1,
                          nullptr, nullptr, st))) return rc;
    if ((rc = launch_sub(d->dtype, d->n_local, d->b, d->q, d->r, d->n_local, 1, st))) return rc;
    if (d->pre.kind != Precond::kNone) {      // z0 = M^-1 r0, d = z0, rho0 = all-reduced r0.z0, history[0] = r0.r0
        if (d->pre.kind == Precond::kMg && d->n_pad > d->n_local)      // the cycle reads whole packs of r: nothing else ever writes the padding
            CG_HIP(hipMemsetAsync(static_cast<char *>(d->r) + vb, 0, (size_t)(d->n_pad - d->n_local) * vs, st));
        if ((rc = pcg_sweep(d, false, d->d_ext, st))) return rc;
        if ((rc = pcg_reduce2(d, 1, st))) return rc;
    } else {
        CG_HIP(hipMemcpyAsync(d->d_ext, d->r, vb, hipMemcpyDeviceToDevice, st));
        if ((rc = launch_dot_partials(d->dtype, d->n_local, d->r, d->r, d->n_local, 1, d->part_rr, d->vgrid, st))) return rc;
        if ((rc = reduce_all(d, d->part_rr, d->vgrid, 1, 1, st))) return rc;
    }
    if (d->cg1) {       // the residual lives in d_ext; p = s = 0 (the first iteration runs with beta = 0)
        CG_HIP(hipMemsetAsync(d->r, 0, vb, st));
        CG_HIP(hipMemsetAsync(d->s2, 0, vb, st));
    }
    d->rhs_set = true;
    d->iters = 0;
    d->stop.armed = d->until_stopped = false;
    return CGAMD_OK;
}

int cgamd_dist_iterate(cgamd_dist *d, int nIterations) {
    if (!d) return fail(CGAMD_ERR_INVALID, "dist_iterate: null handle");
    TuneScope ts(&d->tune);
    if (!d->rhs_set) return fail(CGAMD_ERR_STATE, "dist_iterate: call dist_set_rhs first");
    if (nIterations < 0) return fail(CGAMD_ERR_INVALID, "dist_iterate: negative iteration count");
    if (d->until_stopped) return fail(CGAMD_ERR_STATE, "dist_iterate: dist_iterate_until has stopped the handle: call dist_set_rhs");
    CG_HIP(hipSetDevice(d->ctx->device));
    if (int rc = ensure_history(d, d->iters + nIterations + 1)) return rc;
    hipStream_t st = d->ctx->stream;
    int left = nIterations;
    // (the slab loop has no preconditioned form: such a handle runs its launched loop while a preconditioner is set)
    if (d->slab.ok && d->pre.kind == Precond::kNone && nIterations >= std::max(1, d->tune.resident_wide_min)) {
        // the whole call in one launch per 2^15 iterations (slab.hip); same state in and out as the launched loop below
        while (left > 0) {
            const int K = std::min(left, 1 << 15);
            bool untouched = false;
            if (int rc = run_cg_slab(d->dtype, d->slab, d->n_local, d->nnz, d->vals, d->ptr, d->codes, d->dict, d->x, d->r, d->d_ext,
                                     d->ds[0], d->ds[1], d->slab_comm.mailbox ? &d->slab_comm : nullptr, d->sc, d->iters, K, d->slab_sync, st,
                                     &untouched)) {
                // with peers the launched loops speak another protocol than the peers' slab launches: no silent change of loop
                if (!untouched || d->nranks > 1 || !d->peer.empty()) return rc;
                d->slab.ok = false;          // the chip is shared with something that does not yield: launched loop from here on
                break;
            }
            d->iters += K;
            left -= K;
        }
        if (left == 0) return CGAMD_OK;
        nIterations = left;
    }
    // Optional hipGraph replay of one iteration including the RCCL operations (RCCL >= 2.9 captures).
    if ((d->flags & CGAMD_DIST_GRAPH) && !d->graph_failed && !d->gexec) {
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed);
        int rc = e == hipSuccess ? enqueue_iteration(d, st) : CGAMD_ERR_HIP;
        hipError_t e2 = hipStreamEndCapture(st, &d->graph);
        if (e != hipSuccess || rc != CGAMD_OK || e2 != hipSuccess ||
            hipGraphInstantiate(&d->gexec, d->graph, nullptr, nullptr, 0) != hipSuccess) {
            d->graph_failed = true;
            d->gexec = nullptr;
            (void)hipGetLastError();
        }
    }
    for (; left > 0; --left) {
        if (d->gexec) CG_HIP(hipGraphLaunch(d->gexec, st));
        else if (int rc = enqueue_iteration(d, st)) return rc;
    }
    d->iters += nIterations;
    if (d->cg1 && nIterations > 0) return enqueue_tail_cg1(d, st);
    return CGAMD_OK;
}

// Tolerance stop ON THE DEVICE for the launched loops of the row-partitioned handle (include/cgamd.h): the single-right-hand-side case
// of cgamd_solver_iterate_until, decided from the GLOBALLY reduced r.r -- bit-identical on every rank, so all ranks stop in the same
// iteration without a further exchange, and every rank enqueues the same chunks because each waits for the word of a specific chunk
// at a specific point of its enqueue sequence.  Iterations enqueued after the stop keep the whole protocol running and change
// nothing (enqueue_iteration with the record), so the result does not depend on checkEvery, and until(a); until(b) leaves the bits of
// until(a + b).
int cgamd_dist_iterate_until(cgamd_dist *d, int maxIterations, double tol, int checkEvery, int *iterations_run) {
    if (maxIterations < 0 || checkEvery < 0) return fail(CGAMD_ERR_INVALID, "dist_iterate_until: negative maxIterations or checkEvery");
    if (!(tol > 0.)) return fail(CGAMD_ERR_INVALID, "dist_iterate_until: the tolerance must be positive");
    if (!d || !iterations_run) return fail(CGAMD_ERR_INVALID, "dist_iterate_until: NULL handle or iterations_run");
    TuneScope ts(&d->tune);
    if (!d->rhs_set) return fail(CGAMD_ERR_STATE, "dist_iterate_until: call dist_set_rhs first");
    if (d->cg1)
        return fail(CGAMD_ERR_STATE, "dist_iterate_until: the single-reduction loop (CGAMD_DIST_SINGLE_REDUCTION) runs another recurrence and a "
                                     "tail launch per call; it has no guarded form");
    if (d->p2p && !d->p2p_attached) return fail(CGAMD_ERR_STATE, "p2p backend: call cgamd_dist_attach_p2p first");
    if (maxIterations == 0 || d->until_stopped) {
        *iterations_run = d->iters;
        return CGAMD_OK;
    }
    CG_HIP(hipSetDevice(d->ctx->device));
    hipStream_t st = d->ctx->stream;
    if (int rc = stop_run_alloc(d->stop, 1)) return rc;
    if (int rc = ensure_history(d, d->iters + maxIterations + 1)) return rc;
    if (int rc = stop_run_arm(d->stop, &tol, 1, st)) return rc;
    // (plain launches, every rank the same chunks: each waits for the word of a specific chunk at a specific point of its sequence)
    auto enqueue = [&](int len) -> int {
        for (int i = 0; i < len; ++i)
            if (int rc = enqueue_iteration(d, st, &d->stop.view)) return rc;
        return CGAMD_OK;
    };
    if (int rc = stop_run_chunks(d->stop, maxIterations, checkEvery ? checkEvery : 8, st, enqueue)) {
        const std::string why = cgamd_last_error();     // part of an iteration may be in the stream: the handle demands a fresh set_rhs
        (void)hipStreamSynchronize(st);
        d->rhs_set = false;
        return fail(rc, why);
    }
    if (int rc = stop_run_read(d->stop, st)) return rc;
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) { d->rhs_set = false; return fail(CGAMD_ERR_HIP, std::string("dist_iterate_until: ") + hipGetErrorString(e)); }
    if (const int perr = cgamd_dist_p2p_error(d)) {
        d->rhs_set = false;
        return fail(CGAMD_ERR_COMM, "dist_iterate_until: a bounded spin of the peer-to-peer protocol timed out (error word " + std::to_string(perr) + ")");
    }
    const int stopped_at = d->stop.stopped[0];
    if (stopped_at) { d->iters = stopped_at; d->until_stopped = true; }
    else d->iters += d->stop.enqueued;
    *iterations_run = d->iters;
    return CGAMD_OK;
}

int cgamd_dist_iterations_done(cgamd_dist *d) {
    if (!d) { fail(CGAMD_ERR_INVALID, "dist_iterations_done: null handle"); return -CGAMD_ERR_INVALID; }
    if (!d->rhs_set) { fail(CGAMD_ERR_STATE, "dist_iterations_done: no right-hand side set"); return -CGAMD_ERR_STATE; }
    return d->iters;
}

// ---- preconditioners.  Collective in meaning, local in execution: nothing here communicates.  They take effect at the next
// cgamd_dist_set_rhs; a failed call leaves the handle as it was.
static void drop_graph(cgamd_dist *d) {
    if (d->gexec) { (void)hipGraphExecDestroy(d->gexec); d->gexec = nullptr; }
    if (d->graph) { (void)hipGraphDestroy(d->graph); d->graph = nullptr; }
}
// M has just been replaced or removed: the captured graph replays the old loop, the recurrence starts again at set_rhs, and a cut
// matrix whose hierarchy is gone goes too
static void pre_replaced(cgamd_dist *d) {
    if (!d->pre.mg) free_cut(&d->cut);
    drop_graph(d);
    d->rhs_set = false;
}
static void drop_preconditioner(cgamd_dist *d) {
    precond_drop(&d->pre);
    pre_replaced(d);
}
static int pre_begin(cgamd_dist *d, const char *who) {
    if (d->cg1)
        return fail(CGAMD_ERR_STATE, std::string(who) + ": the single-reduction loop (CGAMD_DIST_SINGLE_REDUCTION) has no PCG form");
    CG_HIP(hipSetDevice(d->ctx->device));
    CG_HIP(hipStreamSynchronize(d->ctx->stream));
    return CGAMD_OK;
}
// what the diagonal and multigrid loops need besides M: vgrid pairs of partials and the rho parity buffer
static int pre_buffers(cgamd_dist *d) {
    if (!d->part_pcg)
        if (int rc = dmalloc(&d->part_pcg, 2 * acc_size(d->dtype) * (size_t)d->vgrid, "partials_rz/rr")) return rc;
    return precond_ensure_rho(&d->pre, d->dtype, 1);
}
// the handle takes m (n_local device values, its own allocation from here on) over
static int install_diag(cgamd_dist *d, void *m, Precond::Built built) {
    if (int rc = pre_buffers(d)) {
        (void)hipFree(m);
        return rc;
    }
    precond_take_diag(&d->pre, m, built);
    pre_replaced(d);
    return CGAMD_OK;
}

int cgamd_dist_set_preconditioner(cgamd_dist *d, const void *m_local) {
    if (!d) return fail(CGAMD_ERR_INVALID, "dist_set_preconditioner: null handle");
    TuneScope ts(&d->tune);
    if (!m_local) {
        CG_HIP(hipSetDevice(d->ctx->device));
        CG_HIP(hipStreamSynchronize(d->ctx->stream));
        drop_preconditioner(d);
        return CGAMD_OK;
    }
    if (int rc = pre_begin(d, "dist_set_preconditioner")) return rc;
    const size_t vb = (size_t)d->n_local * dtype_size(d->dtype);
    void *m = nullptr;
    if (int rc = dmalloc(&m, vb, "preconditioner")) return rc;
    hipError_t e = hipMemcpyAsync(m, m_local, vb, hipMemcpyDeviceToDevice, d->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->ctx->stream);
    if (e != hipSuccess) { (void)hipFree(m); return fail(CGAMD_ERR_HIP, std::string("dist_set_preconditioner: ") + hipGetErrorString(e)); }
    return install_diag(d, m, Precond::kCaller);
}

int cgamd_dist_set_preconditioner_jacobi(cgamd_dist *d) {
    if (!d) return fail(CGAMD_ERR_INVALID, "dist_set_preconditioner_jacobi: null handle");
    TuneScope ts(&d->tune);
    if (int rc = pre_begin(d, "dist_set_preconditioner_jacobi")) return rc;
    void *m = nullptr;
    if (int rc = dmalloc(&m, (size_t)d->n_local * dtype_size(d->dtype), "Jacobi preconditioner")) return rc;
    // the diagonal of local row i is local column i: the halo columns (>= n_local) never match a row
    if (int rc = jacobi_build_from_matrix(d->ctx->stream, d->dtype, d->n_local, "dist_set_preconditioner_jacobi", d->vals, d->ptr, d->cols, m)) {
        (void)hipFree(m);
        return rc;
    }
    return install_diag(d, m, Precond::kJacobi);
}

int cgamd_dist_set_preconditioner_line(cgamd_dist *d, int stride) {
    if (!d) return fail(CGAMD_ERR_INVALID, "dist_set_preconditioner_line: null handle");
    TuneScope ts(&d->tune);
    if (int rc = pre_begin(d, "dist_set_preconditioner_line")) return rc;
    if (stride < 1 || stride >= d->n_local) return fail(CGAMD_ERR_INVALID, "dist_set_preconditioner_line: stride must be in [1, size - 1]");
    // only columns below n_local count: halo slot h is local column n_local + h, and row n_local - 1 - k coupled to a halo slot would
    // otherwise pass for a line neighbour at the right distance.  Lines therefore end at the rank's row range.
    TriBuilt b;
    int rc = tri_build_from_matrix(d->ctx->stream, d->dtype, d->n_local, d->n_local, d->tune.dev_line_host_route, "dist_set_preconditioner_line",
                                   stride, d->vals, d->ptr, d->cols, d->n_local, &b);
    if (rc) return rc;
    if ((rc = precond_take_tri(&d->pre, &b, d->dtype, 1, 0, stride))) return rc;
    pre_replaced(d);
    return CGAMD_OK;
}

// ---- multigrid on the cut matrix (include/cgamd.h).  The cut matrix: count, scan, fill (dist_cut.hip), its row pointers extended by
// the empty padding rows, 64 zeroed entries behind columns and values as the coarse levels carry, and a plan made as theirs is.  It
// runs the as-passed SpMV: the handle's column / value codes describe the uncut rows.
static int build_cut(cgamd_dist *d, const std::string &who, cgamd_dist::CutMatrix *out) {
    const int dt = d->dtype, nu = d->n_local, n = d->n_pad;
    const size_t vs = dtype_size(dt);
    hipStream_t st = d->ctx->stream;
    cgamd_dist::CutMatrix c;
    void *words = nullptr;      // ints: [0] scan overflow flag, [4 ...] scratch of compute_spmv_plan
    int rc = dmalloc(&words, 64, "cut matrix: setup words");
    int *flag = static_cast<int *>(words), *scratch = flag + 4;
    if (!rc) rc = dmalloc((void **)&c.ptr, ((size_t)n + 1 + 64) * 4, "cut matrix: row pointers");
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemsetAsync(words, 0, 64, st);
    if (!rc && e == hipSuccess) rc = launch_cut_count(nu, n, nu, d->ptr, d->cols, c.ptr, st);
    if (!rc && e == hipSuccess) rc = launch_mg_scan(n, c.ptr, flag, st);
    int back[2] = {0, 0};       // overflow flag, kept entries
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(&back[0], flag, 4, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(&back[1], c.ptr + n, 4, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(st);
    if (!rc && e == hipSuccess && (back[0] || back[1] < 0 || back[1] > d->nnz)) rc = fail(CGAMD_ERR_HIP, who + ": the cut matrix's entry count is out of range");
    if (!rc && e == hipSuccess) {
        c.nnz = back[1];
        rc = dmalloc((void **)&c.cols, ((size_t)c.nnz + 64) * 4, "cut matrix: columns");
        if (!rc) rc = dmalloc(&c.vals, ((size_t)c.nnz + 64) * vs, "cut matrix: values");
        if (!rc) e = hipMemsetAsync(c.cols, 0, ((size_t)c.nnz + 64) * 4, st);
        if (!rc && e == hipSuccess) e = hipMemsetAsync(c.vals, 0, ((size_t)c.nnz + 64) * vs, st);
        if (!rc && e == hipSuccess) rc = launch_cut_fill(dt, nu, nu, d->vals, d->ptr, d->cols, c.ptr, c.cols, c.vals, st);
        if (!rc && e == hipSuccess) {
            c.plan = make_spmv_plan(n);
            rc = compute_spmv_plan(c.ptr, c.cols, n, scratch, st, &c.plan);
            if (!rc) finalize_spmv_plan(&c.plan, dt, 1, n, c.nnz, c.vals, c.cols);
        }
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (words) (void)hipFree(words);
    if (!rc && e != hipSuccess) rc = fail(CGAMD_ERR_HIP, who + ": cut matrix: " + hipGetErrorString(e));
    if (rc) { free_cut(&c); return rc; }
    *out = c;
    return CGAMD_OK;
}

// refresh = false: a new cut matrix and hierarchy, installed when both stand (a failure leaves the handle as it was).  refresh = true
// (cgamd_dist_refresh_values): the pattern in place, its values refilled from the rank's, the hierarchy built again on them
static int multigrid_from_cut(cgamd_dist *d, const std::string &who, const MgParams &p, bool refresh) {
    hipStream_t st = d->ctx->stream;
    cgamd_dist::CutMatrix c;
    int rc;
    if (refresh) {
        c = d->cut;
        if ((rc = launch_cut_refill(d->dtype, d->n_local, d->n_local, d->vals, d->ptr, d->cols, c.ptr, c.vals, st))) return rc;
    } else if ((rc = build_cut(d, who, &c))) return rc;
    MgHierarchy *h = nullptr;
    rc = mg_build(st, d->dtype, d->n_local, d->n_pad, 1, 0, c.plan, c.nnz, c.vals, c.ptr, c.cols, p, who, &h);
    if (!rc && (rc = pre_buffers(d))) mg_free(h);
    if (rc) {
        if (!refresh) free_cut(&c);
        return rc;
    }
    if (!refresh) free_cut(&d->cut);        // (the cut matrix of the hierarchy that goes, if any)
    precond_take_mg(&d->pre, h, p);
    d->cut = c;
    pre_replaced(d);
    return CGAMD_OK;
}
static int mg_begin(cgamd_dist *d, const std::string &who) {
    if (int rc = pre_begin(d, who.c_str())) return rc;
    if (d->n_pad % (int)(16 / dtype_size(d->dtype)) != 0) return fail(CGAMD_ERR_INVALID, who + ": the rank has too many rows for the padding to whole 16-byte packs");
    return CGAMD_OK;
}

int cgamd_dist_set_preconditioner_multigrid(cgamd_dist *d, int nx, int ny, int nz, int smooth_steps, double over_correction, int min_rows) {
    const std::string who = "dist_set_preconditioner_multigrid";
    if (!d) return fail(CGAMD_ERR_INVALID, who + ": null handle");
    TuneScope ts(&d->tune);
    if (int rc = mg_begin(d, who)) return rc;
    MgParams p;
    if (int rc = mg_params_grid(who, d->n_local, " (the rank's own box: n_local rows)", nx, ny, nz, smooth_steps, over_correction, min_rows, &p)) return rc;
    return multigrid_from_cut(d, who, p, false);
}

int cgamd_dist_set_preconditioner_amg(cgamd_dist *d, int passes, double strength, int smooth_steps, double over_correction, int min_rows) {
    const std::string who = "dist_set_preconditioner_amg";
    if (!d) return fail(CGAMD_ERR_INVALID, who + ": null handle");
    TuneScope ts(&d->tune);
    if (int rc = mg_begin(d, who)) return rc;
    MgParams p;
    if (int rc = mg_params_amg(who, passes, strength, smooth_steps, over_correction, min_rows, &p)) return rc;
    return multigrid_from_cut(d, who, p, false);
}

int cgamd_dist_mg_levels(cgamd_dist *d) {
    if (!d) return -CGAMD_ERR_INVALID;
    return d->pre.mg ? mg_levels(d->pre.mg) : 0;
}
static int dist_mg_wanted(cgamd_dist *d, const char *who) {
    if (!d) return fail(CGAMD_ERR_INVALID, std::string(who) + ": null handle");
    if (!d->pre.mg) return fail(CGAMD_ERR_STATE, std::string(who) + ": no multigrid preconditioner is set");
    CG_HIP(hipSetDevice(d->ctx->device));
    return CGAMD_OK;
}
int cgamd_dist_mg_level(cgamd_dist *d, int level, long long info[6]) {
    if (int rc = dist_mg_wanted(d, "dist_mg_level")) return rc;
    if (!info) return fail(CGAMD_ERR_INVALID, "dist_mg_level: info is NULL");
    return mg_level_info(d->pre.mg, level, info);
}
int cgamd_dist_mg_level_matrix(cgamd_dist *d, int level, int *ptr, int *cols, void *vals) {
    if (int rc = dist_mg_wanted(d, "dist_mg_level_matrix")) return rc;
    return mg_level_matrix(d->pre.mg, level, ptr, cols, vals, d->ctx->stream);
}
// one V-cycle on caller vectors (n_local device values each), through buffers with the padding rows; synchronises
int cgamd_dist_mg_apply(cgamd_dist *d, const void *r_dev, void *z_dev) {
    if (int rc = dist_mg_wanted(d, "dist_mg_apply")) return rc;
    if (!r_dev || !z_dev) return fail(CGAMD_ERR_INVALID, "dist_mg_apply: null argument");
    TuneScope ts(&d->tune);
    if (int rc = stream_not_capturing(d->ctx->stream, "dist_mg_apply")) return rc;
    return mg_apply_padded(d->pre.mg, d->ctx->stream, d->dtype, d->n_pad, d->n_local, 1, r_dev, z_dev, "dist_mg_apply");
}

// a preconditioner built from the rank's matrix follows its values: removed where the values' own follow-up failed with status rc
// (text in cgamd_last_error()) -- they are in force, read as they are, and factors of the old ones must not stay --
static int remove_and_fail(cgamd_dist *d, int rc) {
    if (d->pre.built == Precond::kCaller) return rc;
    const std::string why = cgamd_last_error();
    drop_preconditioner(d);
    return fail(rc, why);
}
// -- and built again from the values as they are now, or removed where that fails
static int rebuild_or_remove(cgamd_dist *d) {
    int rc = CGAMD_OK;
    switch (d->pre.built) {
    case Precond::kCaller: return CGAMD_OK;
    case Precond::kJacobi: rc = cgamd_dist_set_preconditioner_jacobi(d); break;
    case Precond::kLine: rc = cgamd_dist_set_preconditioner_line(d, d->pre.stride); break;
    case Precond::kGridMg:
    case Precond::kAmg: {
        const MgParams p = d->pre.mg_params;
        rc = multigrid_from_cut(d, p.algebraic ? "dist_set_preconditioner_amg" : "dist_set_preconditioner_multigrid", p, true);
    } break;
    }
    return rc ? remove_and_fail(d, rc) : CGAMD_OK;
}

// The rank's matrix values changed in place on the same pattern (include/cgamd.h).  Rank-local: nothing here communicates; collective
// in meaning: every rank calls it.  What was made from the values follows them: the value codes (dictionary rewritten in place where
// the equal-value classes are intact, else rebuilt or dropped, with the captured graph) and a preconditioner built from the matrix.
int cgamd_dist_refresh_values(cgamd_dist *d) {
    if (!d) return fail(CGAMD_ERR_INVALID, "dist_refresh_values: null handle");
    TuneScope ts(&d->tune);
    CG_HIP(hipSetDevice(d->ctx->device));
    hipStream_t st = d->ctx->stream;
    if (int rc = stream_not_capturing(st, "dist_refresh_values")) return rc;
    CG_HIP(hipStreamSynchronize(st));
    d->rhs_set = false;
    d->last_refresh = 0;
    if (value_codes_apply(d) && d->nnz > 0) {
        bool kept = false;
        int rc = CGAMD_OK;
        if (d->vcodes) rc = refresh_value_dicts(d->dtype, d->nnz, d->vals, d->vcodes, d->vdict, 0, nullptr, nullptr, 0, nullptr, st, &kept);
        if (!rc && kept) d->last_refresh = 1;
        else {
            const bool had = d->vcodes != nullptr;
            drop_value_codes(d);
            if (!rc) rc = setup_value_codes(d);
            if (rc) drop_value_codes(d);
            if (had || d->vcodes) drop_graph(d);        // the captured launches hold the old array, or read aValues
            if (rc) {       // the values are in force, read as they are; factors of the old ones must not stay
                d->last_refresh = -rc;
                return remove_and_fail(d, rc);
            }
            d->last_refresh = d->vcodes ? 2 : 3;
        }
    }
    return rebuild_or_remove(d);
}
int cgamd_dist_last_refresh(cgamd_dist *d) { return d ? d->last_refresh : -CGAMD_ERR_INVALID; }

int cgamd_dist_get_x(cgamd_dist *d, void *x_local) {
    if (!d || !x_local) return fail(CGAMD_ERR_INVALID, "dist_get_x: null argument");
    CG_HIP(hipSetDevice(d->ctx->device));
    CG_HIP(hipMemcpyAsync(x_local, d->x, (size_t)d->n_local * dtype_size(d->dtype), hipMemcpyDeviceToDevice, d->ctx->stream));
    return CGAMD_OK;
}

int cgamd_dist_history(cgamd_dist *d, void *history, int max_entries) {
    if (!d || !history) { fail(CGAMD_ERR_INVALID, "dist_history: null argument"); return -CGAMD_ERR_INVALID; }
    if (!d->rhs_set) { fail(CGAMD_ERR_STATE, "dist_history: no right-hand side set"); return -CGAMD_ERR_STATE; }
    if (hipSetDevice(d->ctx->device) != hipSuccess) return -CGAMD_ERR_NO_DEVICE;
    const int entries = std::min(std::min(d->iters + 1, d->sc.history_cap), max_entries);
    hipError_t e = hipMemcpyAsync(history, d->sc.history, (size_t)entries * dtype_size(d->dtype), hipMemcpyDeviceToHost, d->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->ctx->stream);
    if (e != hipSuccess) { fail(CGAMD_ERR_HIP, std::string("dist_history: ") + hipGetErrorString(e)); return -CGAMD_ERR_HIP; }
    return entries;
}

int cgamd_dist_synchronize(cgamd_dist *d) {
    if (!d) return fail(CGAMD_ERR_INVALID, "dist_synchronize: null handle");
    CG_HIP(hipSetDevice(d->ctx->device));
    CG_HIP(hipStreamSynchronize(d->ctx->stream));
    return CGAMD_OK;
}

// ---- peer-to-peer backend: mailbox allocation and attachment -------------------------------------------
int cgamd_p2p_mailbox_alloc(cgamd_ctx *ctx, long long halo_values, int dtype, void **mailbox, void *handle64) {
    if (!ctx || !mailbox || !handle64 || halo_values < 0 || dtype < 0 || dtype > 3) return fail(CGAMD_ERR_INVALID, "p2p_mailbox_alloc: bad argument");
    CG_HIP(hipSetDevice(ctx->device));
    const size_t bytes = kMailboxHeader + (size_t)halo_values * dtype_size(dtype) + 256;
    void *p = nullptr;
    hipError_t e = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) return fail(CGAMD_ERR_ALLOC, std::string("hipExtMallocWithFlags(uncached mailbox): ") + hipGetErrorString(e));
    CG_HIP(hipMemset(p, 0, bytes));
    hipIpcMemHandle_t h;
    e = hipIpcGetMemHandle(&h, p);
    if (e != hipSuccess) { (void)hipFree(p); return fail(CGAMD_ERR_HIP, std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e)); }
    static_assert(sizeof(h) == 64, "hipIpcMemHandle_t is 64 bytes");
    memcpy(handle64, &h, 64);
    *mailbox = p;
    return CGAMD_OK;
}

int cgamd_p2p_mailbox_free(cgamd_ctx *ctx, void *mailbox) {
    if (!ctx) return fail(CGAMD_ERR_INVALID, "p2p_mailbox_free: ctx is NULL");
    CG_HIP(hipSetDevice(ctx->device));
    if (mailbox) CG_HIP(hipFree(mailbox));
    return CGAMD_OK;
}

int cgamd_dist_attach_p2p(cgamd_dist *d, void *my_mailbox, const void *handles, const int *dst_offset) {
    if (!d || !my_mailbox || !handles) return fail(CGAMD_ERR_INVALID, "dist_attach_p2p: null argument");
    TuneScope ts(&d->tune);
    if (!d->p2p) return fail(CGAMD_ERR_STATE, "dist_attach_p2p: the handle was not created with CGAMD_DIST_P2P");
    if (d->nranks > 64) return fail(CGAMD_ERR_INVALID, "dist_attach_p2p: at most 64 ranks");
    const int np = (int)d->peer.size();
    if (np > 0 && !dst_offset) return fail(CGAMD_ERR_INVALID, "dist_attach_p2p: dst_offset is NULL");
    CG_HIP(hipSetDevice(d->ctx->device));
    d->my_mailbox = static_cast<char *>(my_mailbox);
    std::vector<char *> base((size_t)d->nranks, nullptr);
    for (int r = 0; r < d->nranks; ++r) {
        if (r == d->rank) { base[(size_t)r] = d->my_mailbox; continue; }
        hipIpcMemHandle_t h;
        memcpy(&h, static_cast<const char *>(handles) + (size_t)r * 64, 64);
        void *m = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&m, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) return fail(CGAMD_ERR_COMM, "hipIpcOpenMemHandle(rank " + std::to_string(r) + "): " + hipGetErrorString(e));
        d->opened.push_back(m);
        base[(size_t)r] = static_cast<char *>(m);
    }
    int rc;
    if ((rc = dmalloc((void **)&d->mailbox_dev, sizeof(char *) * (size_t)d->nranks, "mailbox table"))) return rc;
    CG_HIP(hipMemcpy(d->mailbox_dev, base.data(), sizeof(char *) * (size_t)d->nranks, hipMemcpyHostToDevice));
    d->mailbox_host = base;
    const size_t epoch_bytes = 64 + sizeof(unsigned) * (size_t)(1 + np);   // 3 epochs, then the work-group counters
    if ((rc = dmalloc((void **)&d->epochs, epoch_bytes, "epochs"))) return rc;
    CG_HIP(hipMemset(d->epochs, 0, epoch_bytes));
    std::vector<int> plan((size_t)np * 6 + 1, 0);
    for (int p = 0; p < np; ++p) {
        plan[(size_t)p] = d->peer[(size_t)p];
        plan[(size_t)np + p] = d->send_off[(size_t)p];
        plan[(size_t)2 * np + p] = d->send_count[(size_t)p];
        plan[(size_t)3 * np + p] = dst_offset[p];
        plan[(size_t)4 * np + p] = d->recv_off[(size_t)p];
        plan[(size_t)5 * np + p] = d->recv_count[(size_t)p];
    }
    if ((rc = dmalloc((void **)&d->plan_dev, sizeof(int) * plan.size(), "p2p plan"))) return rc;
    CG_HIP(hipMemcpy(d->plan_dev, plan.data(), sizeof(int) * plan.size(), hipMemcpyHostToDevice));
    d->xch_dst_off.assign(dst_offset, dst_offset + np);
    P2pExchange &x = d->xch;
    x.mailbox = d->mailbox_dev; x.rank = d->rank; x.n_peers = np; x.n_local = d->n_local;
    x.peer_rank = d->plan_dev; x.send_off = d->plan_dev + np; x.send_count = d->plan_dev + 2 * np;
    x.dst_off = d->plan_dev + 3 * np; x.recv_off = d->plan_dev + 4 * np; x.recv_count = d->plan_dev + 5 * np;
    x.send_index = d->send_index; x.epoch = d->epochs;
    x.counters = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(d->epochs) + 64);
    x.my_halo = d->my_mailbox + kMailboxHeader;
    x.max_count = 0;
    for (int p = 0; p < np; ++p) x.max_count = std::max(x.max_count, std::max(d->send_count[(size_t)p], d->recv_count[(size_t)p]));
    if (d->direct && spmv_p2p_grid(d->plan) < np * p2p_push_chunks(x)) d->direct = false;   // too few work-groups to carry the push
    d->p2p_attached = true;
    return CGAMD_OK;
}

// Slab loop (CGAMD_DIST_RESIDENT) on a peer-to-peer handle with peers: d is published in two buffers of n_local + n_halo values that
// live INSIDE every rank's mailbox allocation, behind the halo area, so that the peers can write their boundary entries into the
// tail directly: mailbox = [16 KiB header | n_halo values | ds0 | ds1], each part rounded up to 256 bytes.  mailbox_values: the
// `halo_values` the mailbox was allocated with; rank_n_local / rank_n_halo [nranks]: every rank's sizes (a peer's buffers start
// behind ITS halo area).  Returns CGAMD_OK whether or not the loop applies; cgamd_dist_loop_launches() == 0 tells.
int cgamd_dist_enable_resident(cgamd_dist *d, long long mailbox_values, const int *rank_n_local, const int *rank_n_halo) {
    if (!d || !rank_n_local || !rank_n_halo) return fail(CGAMD_ERR_INVALID, "dist_enable_resident: null argument");
    TuneScope ts(&d->tune);
    if (!d->p2p || !d->p2p_attached) return fail(CGAMD_ERR_STATE, "dist_enable_resident: attach the peer-to-peer mailboxes first");
    if (!d->slab_plan_.ok) return CGAMD_OK;       // nothing to enable (no plan, or the plain buffers of a lone rank are in use)
    CG_HIP(hipSetDevice(d->ctx->device));
    const size_t vs = dtype_size(d->dtype);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    auto ds_off = [&](int r, int which) {       // byte offset of rank r's ds0 / ds1 inside its mailbox
        const size_t halo = up((size_t)rank_n_halo[r] * vs), body = up(((size_t)rank_n_local[r] + rank_n_halo[r]) * vs);
        return kMailboxHeader + halo + (size_t)which * body;
    };
    if (rank_n_local[d->rank] != d->n_local || rank_n_halo[d->rank] != d->n_halo)
        return fail(CGAMD_ERR_INVALID, "dist_enable_resident: sizes of this rank do not match the handle");
    if (ds_off(d->rank, 1) + up(((size_t)d->n_local + d->n_halo) * vs) > kMailboxHeader + (size_t)mailbox_values * vs)
        return fail(CGAMD_ERR_INVALID, "dist_enable_resident: the mailbox allocation is too small for the two published-d buffers");
    const int np = (int)d->peer.size();
    std::vector<void *> dst((size_t)2 * np);
    for (int which = 0; which < 2; ++which)
        for (int p = 0; p < np; ++p) {
            const int q = d->peer[(size_t)p];
            // my entries land at dst_offset[p] of the peer's halo numbering: tail of its buffer
            dst[(size_t)which * np + p] = d->mailbox_host[(size_t)q] + ds_off(q, which) + ((size_t)rank_n_local[q] + d->xch_dst_off[(size_t)p]) * vs;
        }
    int rc;
    if (!d->push_dst_dev && (rc = dmalloc((void **)&d->push_dst_dev, sizeof(void *) * dst.size(), "slab push table"))) return rc;
    CG_HIP(hipMemcpy(d->push_dst_dev, dst.data(), sizeof(void *) * dst.size(), hipMemcpyHostToDevice));
    d->ds[0] = d->my_mailbox + ds_off(d->rank, 0);
    d->ds[1] = d->my_mailbox + ds_off(d->rank, 1);
    SlabComm &c = d->slab_comm;
    c.n_halo = d->n_halo; c.nranks = d->nranks; c.rank = d->rank; c.n_peers = np;
    c.mailbox = d->mailbox_dev;
    c.peer_rank = d->xch.peer_rank; c.send_off = d->xch.send_off; c.send_count = d->xch.send_count; c.recv_count = d->xch.recv_count;
    c.send_index = d->send_index;
    c.push_dst = d->push_dst_dev;
    c.halo_epoch = d->epochs; c.red_seq = d->epochs + 3;
    SlabPlan sp = d->slab_plan_;
    if (np > 0 && d->total_send > 0 && d->tune.slab_trim != 0) {
        // members that push to a peer own fewer rows (slab_partition): try two granules fewer, then one
        std::vector<int> send((size_t)d->total_send);
        CG_HIP(hipMemcpy(send.data(), d->send_index, send.size() * sizeof(int), hipMemcpyDeviceToHost));
        std::vector<char> boundary((size_t)(d->n_local + 1023) / 1024, 0);
        for (int row : send)
            if (row >= 0 && row < d->n_local) boundary[(size_t)row >> 10] = 1;
        {   // ... and the rows that read a peer's entries (they wait for its flag)
            std::vector<int> inner, outer;
            if ((rc = classify_row_blocks(d, &inner, &outer))) return rc;
            for (int rb : outer) boundary[(size_t)rb >> 2] = 1;
        }
        std::vector<int> mstart, gmember;
        const int want = d->tune.slab_trim > 0 ? d->tune.slab_trim : 2;
        for (int trim = std::min(want, sp.rows_m / 1024 - 1); trim >= 1; --trim) {
            const int members = slab_partition(sp, d->n_local, boundary, trim, std::min(d->n_cus, 256), &mstart, &gmember);
            if (members < 2) continue;
            const size_t bytes = (mstart.size() + gmember.size()) * sizeof(int);
            if (d->slab_map) { (void)hipFree(d->slab_map); d->slab_map = nullptr; }
            if ((rc = dmalloc((void **)&d->slab_map, bytes, "slab member map"))) return rc;
            CG_HIP(hipMemcpy(d->slab_map, mstart.data(), mstart.size() * sizeof(int), hipMemcpyHostToDevice));
            CG_HIP(hipMemcpy(d->slab_map + mstart.size(), gmember.data(), gmember.size() * sizeof(int), hipMemcpyHostToDevice));
            sp.mstart = d->slab_map; sp.gmember = d->slab_map + mstart.size(); sp.G = members;
            d->slab_mstart = mstart;
            if (slab_sync_bytes(members) > sp.sync_bytes) {
                if (d->slab_sync) { (void)hipFree(d->slab_sync); d->slab_sync = nullptr; }
                sp.sync_bytes = slab_sync_bytes(members);
                if ((rc = dmalloc(&d->slab_sync, sp.sync_bytes, "slab sync words"))) return rc;
            }
            break;
        }
    }
    d->slab = sp;
    return CGAMD_OK;
}

// ranks of the RCCL communicator this handle runs on, read back from RCCL (0 = no communicator: peer-to-peer backend or
// a single rank without peers); bench.py prints it next to the RCCL timings
int cgamd_dist_comm_ranks(cgamd_dist *d) {
    if (!d || !d->comm) return 0;
    int n = 0;
    if (g_rccl.CommCount(d->comm, &n) != ncclSuccess) return -1;
    return n;
}

// 0 = fine; != 0: a bounded spin of the peer-to-peer protocol timed out (1 boundary exchange, 2 all-reduce)
int cgamd_dist_index_codes(cgamd_dist *d) { return d ? d->n_offsets : -CGAMD_ERR_INVALID; }

// stream operations per iteration of the loop this handle runs (kernel launches, plus RCCL calls with that backend)
int cgamd_dist_loop_launches(cgamd_dist *d) {
    if (!d) return -CGAMD_ERR_INVALID;
    if (d->slab.ok && d->pre.kind == Precond::kNone) return 0;
    if (d->cg1) return d->p2p ? 2 : (d->peer.empty() ? 4 : 6);
    // the preconditioned loops replace launches one for one; the stride-1 line sweep in its long form is three launches, not one
    // multigrid: the r update and the r.z partials are launches of their own around the cycle's chain (one more than the sweep they
    // replace), plus every launch of the cycle
    const int extra = d->pre.kind == Precond::kMg ? 1 + mg_cost(d->pre.mg).launches : (d->pre.kind == Precond::kTri && d->pre.tri.longform) ? 2 : 0;
    if (d->direct && d->p2p_attached) return 4 + extra;
    if (d->p2p) return (d->peer.empty() ? 5 : 7) + extra;
    return (d->peer.empty() ? 9 : 11) + extra;
}

// what the slab loop of this handle runs on: reads the plan in force, launches nothing, changes nothing
int cgamd_dist_slab_plan(cgamd_dist *d, int info[8], int *member_start, int cap) {
    if (!d || !info) return -CGAMD_ERR_INVALID;
    for (int i = 0; i < 8; ++i) info[i] = 0;
    const SlabPlan &sp = d->slab;
    if (!sp.ok || d->pre.kind != Precond::kNone) return 0;
    const bool uniform = sp.mstart == nullptr;
    info[0] = 1; info[1] = sp.G; info[2] = sp.rows_m; info[3] = sp.nsteps; info[4] = sp.unroll; info[5] = sp.nsteps <= 10 ? 10 : 12;
    info[6] = (sp.vcodes && sp.vdict && d->tune.value_codes != 0) ? 1 : 0;
    info[7] = uniform ? 1 : 0;
    if (member_start && cap >= sp.G + 1) {
        for (int m = 0; m <= sp.G; ++m)
            member_start[m] = uniform ? (int)std::min<long long>((long long)m * sp.rows_m, d->n_local) : d->slab_mstart[(size_t)m];
    }
    return sp.G + 1;
}

int cgamd_dist_p2p_error(cgamd_dist *d) {
    if (!d || !d->p2p || !d->my_mailbox) return 0;
    unsigned long long w = 0;
    if (hipSetDevice(d->ctx->device) != hipSuccess) return -1;
    if (hipMemcpy(&w, d->my_mailbox + 6144, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)w;
}

}  // extern "C"
