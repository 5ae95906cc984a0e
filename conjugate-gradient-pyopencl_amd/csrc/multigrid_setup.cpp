// Aggregation multigrid preconditioner on grid systems: the hierarchy of a handle and its V-cycle as a chain of launches
// (cgamd_solver_set_preconditioner_multigrid; kernels in multigrid.hip, the algorithm stated in include/cgamd.h and DESIGN.md).
// The host reads back single words only: the coarse non-zero count, the error words and the Gershgorin bound of every level.
// The algebraic entry (cgamd_solver_set_preconditioner_amg; kernels in amg.hip) builds the same hierarchy with aggregates matched
// from the matrix: its levels carry a stored map and member lists, and the host also reads one word per matching round.
// The batched entry (cgamd_solver_set_preconditioner_batched_multigrid; kernels in multigrid_batched.hip) builds one hierarchy per
// system of a batched handle in the same MgHierarchy (nsys > 0): aggregates, patterns and level vectors shared, values, dinv and
// smoother coefficients per system; the host then reads nsys bound words per level.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cgamd_internal.h"

namespace cgamd {

namespace {
struct MgLevel {
    int n = 0, nu = 0;          // rows the kernels work on (level 0: with the padding rows) / rows of the grid
    long long nnz = 0, ld = 0;
    MgGrid grid;                // this level's dims (nx, ny, nz) and its aggregates' (cnx, cny, cnz)
    const int *agg = nullptr;   // algebraic hierarchy: row -> row of the next level (nu ints), and the members of every aggregate
    const int *mem = nullptr;   // (kAmgWidth ints per row of the next level, ascending, -1 behind the last); nullptr: the box map
    const void *vals = nullptr;
    const int *ptr = nullptr, *cols = nullptr;
    SpmvPlan plan;
    void *dinv = nullptr;       // a batched hierarchy: nsys arrays, system r at r * ld
    double lmax = 0.;           // (a batched hierarchy: the largest of lmaxs)
    void *x = nullptr, *b = nullptr, *w = nullptr, *d = nullptr;      // level 0: x and b are the caller's z and r
    int steps = 1;
    std::vector<double> c0, c1; // Chebyshev coefficients of step k (c0[0] unused); a batched hierarchy: of (step k, system r) at k * nsys + r
    // a batched hierarchy: the bound of every system, and the coefficients rounded to the real type on the device: c0 of step k at
    // coef + 2 k nsys, c1 at coef + (2 k + 1) nsys, nsys values each
    std::vector<double> lmaxs;
    void *coef = nullptr;
    const void *coef0(int k, int nsys, size_t rs) const { return static_cast<const char *>(coef) + (size_t)2 * k * nsys * rs; }
    const void *coef1(int k, int nsys, size_t rs) const { return static_cast<const char *>(coef) + ((size_t)2 * k + 1) * nsys * rs; }
};
}  // namespace

struct MgHierarchy {
    int dtype = 0, nrhs = 1;
    int nsys = 0;               // > 0: a batched handle's hierarchy (nrhs == nsys), one matrix, dinv and smoother per system on every level
    MgParams p;
    std::vector<MgLevel> lv;
    std::vector<void *> owned;
    ~MgHierarchy() {
        for (void *q : owned)
            if (q) (void)hipFree(q);
    }
    int get(void **q, size_t bytes, const char *what) {
        const hipError_t e = hipMalloc(q, bytes ? bytes : 16);
        if (e != hipSuccess)
            return fail(CGAMD_ERR_ALLOC, std::string("hipMalloc(multigrid ") + what + ", " + std::to_string(bytes) + " B): " + hipGetErrorString(e));
        owned.push_back(*q);
        return CGAMD_OK;
    }
};

constexpr double kMgKappaSmooth = 4., kMgKappaCoarsest = 30.;
constexpr int kMgCoarsestSteps = 8;

// the smoother polynomial on [lmax / kappa, lmax]: step 0 scales by 1 / theta, step k by (rho_k rho_{k-1}, 2 rho_k / delta)
static void cheb_coefficients(double lmax, double kappa, int steps, std::vector<double> *c0, std::vector<double> *c1) {
    const double lmin = lmax / kappa, theta = (lmax + lmin) / 2., delta = (lmax - lmin) / 2., sigma = theta / delta;
    c0->assign((size_t)steps, 0.);
    c1->assign((size_t)steps, 0.);
    double rho = 1. / sigma;
    (*c1)[0] = 1. / theta;
    for (int k = 1; k < steps; ++k) {
        const double rho_k = 1. / (2. * sigma - rho);
        (*c0)[(size_t)k] = rho_k * rho;
        (*c1)[(size_t)k] = 2. * rho_k / delta;
        rho = rho_k;
    }
}

// dinv and the Gershgorin bound of a level whose matrix is in place
static int level_diagonal_batched(MgHierarchy *h, MgLevel &L, int level, const std::string &who, hipStream_t st);
static int level_diagonal(MgHierarchy *h, MgLevel &L, int level, unsigned long long *word, const std::string &who, hipStream_t st) {
    if (h->nsys) return level_diagonal_batched(h, L, level, who, st);
    const size_t vs = dtype_size(h->dtype);
    if (int rc = h->get(&L.dinv, (size_t)L.n * vs, "dinv")) return rc;
    CG_HIP(hipMemsetAsync(L.dinv, 0, (size_t)L.n * vs, st));
    if (int rc = jacobi_build_from_matrix(st, h->dtype, L.nu, who + ": level " + std::to_string(level), L.vals, L.ptr, L.cols, L.dinv)) return rc;
    CG_HIP(hipMemsetAsync(word, 0, 8, st));
    if (int rc = launch_mg_gershgorin(h->dtype, L.nu, L.vals, L.ptr, L.dinv, word, st)) return rc;
    unsigned long long bits = 0;
    CG_HIP(hipMemcpyAsync(&bits, word, 8, hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    std::memcpy(&L.lmax, &bits, 8);
    if (!std::isfinite(L.lmax) || !(L.lmax > 0.))
        return fail(CGAMD_ERR_INVALID, who + ": level " + std::to_string(level) + ": the Gershgorin bound of D^-1 A is not a positive finite number");
    return CGAMD_OK;
}

// the same for every system of a batched hierarchy: one launch each for the diagonals and the bounds, one word per system read back
static int level_diagonal_batched(MgHierarchy *h, MgLevel &L, int level, const std::string &who, hipStream_t st) {
    const size_t vs = dtype_size(h->dtype), ns = (size_t)h->nsys;
    void *bounds = nullptr;
    if (int rc = h->get(&L.dinv, (size_t)L.ld * ns * vs, "dinv")) return rc;
    if (int rc = h->get(&bounds, ns * 8, "bound words")) return rc;
    CG_HIP(hipMemsetAsync(L.dinv, 0, (size_t)L.ld * ns * vs, st));
    if (int rc = jacobi_build_from_matrix_batched(st, h->dtype, L.nu, h->nsys, L.nnz, who, L.vals, L.ptr, L.cols, L.dinv, L.ld, level)) return rc;
    CG_HIP(hipMemsetAsync(bounds, 0, ns * 8, st));
    if (int rc = launch_mg_gershgorin_batched(h->dtype, L.nu, h->nsys, L.nnz, L.ld, L.vals, L.ptr, L.dinv,
                                              static_cast<unsigned long long *>(bounds), st)) return rc;
    L.lmaxs.assign(ns, 0.);
    CG_HIP(hipMemcpyAsync(L.lmaxs.data(), bounds, ns * 8, hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    L.lmax = 0.;
    for (size_t r = 0; r < ns; ++r) {
        if (!std::isfinite(L.lmaxs[r]) || !(L.lmaxs[r] > 0.))
            return fail(CGAMD_ERR_INVALID, who + ": system " + std::to_string(r) + " level " + std::to_string(level) +
                                               ": the Gershgorin bound of D^-1 A is not a positive finite number");
        L.lmax = std::max(L.lmax, L.lmaxs[r]);
    }
    return CGAMD_OK;
}

// the plan of a coarse level's batched product: what a batched handle's own plan holds (one d.q partial slot per 256-row block, the
// cache policy priced on all value arrays)
static void batched_level_plan(SpmvPlan *plan, int dt, int nsys, int n, long long nnz) {
    plan->n_partials = plan->row_blocks;
    const size_t V = dtype_size(dt), MB = (size_t)1 << 20;
    const size_t matrix_bytes = (size_t)nnz * (V * (size_t)nsys + 4) + ((size_t)n + 1) * 4;
    plan->nt = tune().spmv_nt >= 0 ? (tune().spmv_nt != 0) : (matrix_bytes > 256 * MB);
}

namespace {
// device memory of one level's setup: freed when the level is done, but for what the hierarchy keeps
struct AmgTemps {
    std::vector<void *> v;
    ~AmgTemps() {
        for (void *q : v)
            if (q) (void)hipFree(q);
    }
    int get(void **q, size_t bytes, const char *what) {
        const hipError_t e = hipMalloc(q, bytes ? bytes : 16);
        if (e != hipSuccess)
            return fail(CGAMD_ERR_ALLOC, std::string("hipMalloc(amg ") + what + ", " + std::to_string(bytes) + " B): " + hipGetErrorString(e));
        v.push_back(*q);
        return CGAMD_OK;
    }
    void drop(void *q) {
        for (void *&t : v)
            if (t && t == q) { (void)hipFree(t); t = nullptr; }
    }
    void keep(void *q, MgHierarchy *h) {
        for (void *&t : v)
            if (t && t == q) { h->owned.push_back(t); t = nullptr; }
    }
};
}  // namespace

// The next level of an algebraic hierarchy from its last level: up to p.passes passes of handshake matching, each on the Galerkin
// product of the pass before; the passes kept give the composed map, the member lists and the coarse matrix (the last kept product).
// *built = false: the level is not built (no pass kept, or the rows fall to more than 0.8 of the fine rows) and the hierarchy ends
static int amg_coarsen(MgHierarchy *h, unsigned long long *word, int *flag, const std::string &who, hipStream_t st, MgLevel *C, bool *built) {
    *built = false;
    const int dt = h->dtype, level = (int)h->lv.size();
    const size_t vs = dtype_size(dt);
    MgLevel &F = h->lv.back();
    const int nf = F.nu;
    AmgTemps tmp;
    void *smax = nullptr, *match = nullptr, *pick = nullptr, *rank = nullptr, *pmap = nullptr, *pairs = nullptr, *agg = nullptr, *formed = nullptr;
    if (int rc = tmp.get(&smax, (size_t)nf * 8, "row maxima")) return rc;
    if (int rc = tmp.get(&match, (size_t)nf * 4, "matching")) return rc;
    if (int rc = tmp.get(&pick, (size_t)nf * 4, "picks")) return rc;
    if (int rc = tmp.get(&rank, ((size_t)nf + 1) * 4, "ranks")) return rc;
    if (int rc = tmp.get(&pmap, (size_t)nf * 4, "pass map")) return rc;
    if (int rc = tmp.get(&pairs, (size_t)nf * 8, "pairs")) return rc;
    if (int rc = tmp.get(&agg, (size_t)nf * 4, "map")) return rc;
    if (int rc = tmp.get(&formed, 16, "round word")) return rc;

    const void *vals = F.vals;
    const int *ptr = F.ptr, *cols = F.cols;
    int n = nf, kept = 0;
    long long nnz = F.nnz;
    void *mem = nullptr, *kp = nullptr, *kc = nullptr, *kv = nullptr;       // the member lists and the product of the passes kept
    for (int pass = 0; pass < h->p.passes; ++pass) {
        if (int rc = launch_amg_smax(dt, n, vals, ptr, cols, static_cast<double *>(smax), st)) return rc;
        CG_HIP(hipMemsetAsync(match, 0xff, (size_t)n * 4, st));
        for (int round = 0; round < kAmgMaxRounds; ++round) {
            CG_HIP(hipMemsetAsync(formed, 0, 4, st));
            if (int rc = launch_amg_pick(dt, n, h->p.theta, vals, ptr, cols, static_cast<const double *>(smax), static_cast<const int *>(match),
                                         static_cast<int *>(pick), st)) return rc;
            if (int rc = launch_amg_handshake(n, static_cast<const int *>(pick), static_cast<int *>(match), static_cast<int *>(formed), st)) return rc;
            int any = 0;
            CG_HIP(hipMemcpyAsync(&any, formed, 4, hipMemcpyDeviceToHost, st));
            CG_HIP(hipStreamSynchronize(st));
            if (!any) break;        // (a round that forms no pair leaves the state to the next one as it found it)
        }
        CG_HIP(hipMemsetAsync(flag, 0, 4, st));
        if (int rc = launch_amg_roots(n, static_cast<const int *>(match), static_cast<int *>(rank), st)) return rc;
        if (int rc = launch_mg_scan(n, static_cast<int *>(rank), flag, st)) return rc;
        if (int rc = launch_amg_number(n, static_cast<const int *>(match), static_cast<const int *>(rank), static_cast<int *>(pmap),
                                       static_cast<int *>(pairs), st)) return rc;
        int nc = 0;
        CG_HIP(hipMemcpyAsync(&nc, static_cast<int *>(rank) + n, 4, hipMemcpyDeviceToHost, st));
        CG_HIP(hipStreamSynchronize(st));
        if (nc < 1 || nc > n) return fail(CGAMD_ERR_HIP, who + ": level " + std::to_string(level) + ": the aggregate count is out of range");
        // the product of the pass: rows from the pairs, columns through the pass map
        void *ptrc = nullptr, *colsc = nullptr, *valsc = nullptr;
        if (int rc = tmp.get(&ptrc, ((size_t)nc + 1 + 64) * 4, "row pointers")) return rc;
        CG_HIP(hipMemsetAsync(word, 0xff, 8, st));
        CG_HIP(hipMemsetAsync(flag, 0, 4, st));
        if (int rc = launch_amg_count(nc, 2, static_cast<const int *>(pairs), static_cast<const int *>(pmap), ptr, cols, static_cast<int *>(ptrc),
                                      word, st)) return rc;
        if (int rc = launch_mg_scan(nc, static_cast<int *>(ptrc), flag, st)) return rc;
        unsigned long long err_h = 0;
        int back[2] = {0, 0};     // overflow flag, coarse nnz
        CG_HIP(hipMemcpyAsync(&err_h, word, 8, hipMemcpyDeviceToHost, st));
        CG_HIP(hipMemcpyAsync(&back[0], flag, 4, hipMemcpyDeviceToHost, st));
        CG_HIP(hipMemcpyAsync(&back[1], static_cast<int *>(ptrc) + nc, 4, hipMemcpyDeviceToHost, st));
        CG_HIP(hipStreamSynchronize(st));
        if (err_h != ~0ull) break;      // a row of more than kMgMaxRow columns: this pass and the ones after it are dropped
        if (back[0]) return fail(CGAMD_ERR_INVALID, who + ": level " + std::to_string(level) + ": the coarse matrix has more than 2^31 - 1 entries");
        const long long nnzc = back[1];
        if (int rc = tmp.get(&colsc, ((size_t)nnzc + 64) * 4, "columns")) return rc;
        if (int rc = tmp.get(&valsc, ((size_t)nnzc + 64) * vs, "values")) return rc;
        CG_HIP(hipMemsetAsync(colsc, 0, ((size_t)nnzc + 64) * 4, st));
        CG_HIP(hipMemsetAsync(valsc, 0, ((size_t)nnzc + 64) * vs, st));
        if (int rc = launch_amg_fill(dt, nc, 2, static_cast<const int *>(pairs), static_cast<const int *>(pmap), vals, ptr, cols,
                                     static_cast<const int *>(ptrc), static_cast<int *>(colsc), valsc, st)) return rc;
        // the pass is kept: the level's map and member lists take it in
        void *mem_new = nullptr;
        if (int rc = tmp.get(&mem_new, (size_t)nc * kAmgWidth * 4, "member lists")) return rc;
        if (int rc = launch_amg_compose(nf, static_cast<const int *>(pmap), kept ? static_cast<const int *>(agg) : nullptr, static_cast<int *>(agg), st)) return rc;
        if (int rc = launch_amg_members(nc, static_cast<const int *>(pairs), static_cast<const int *>(mem), static_cast<int *>(mem_new), st)) return rc;
        CG_HIP(hipStreamSynchronize(st));
        tmp.drop(mem); tmp.drop(kp); tmp.drop(kc); tmp.drop(kv);
        mem = mem_new; kp = ptrc; kc = colsc; kv = valsc;
        vals = valsc; ptr = static_cast<const int *>(ptrc); cols = static_cast<const int *>(colsc);
        n = nc; nnz = nnzc;
        ++kept;
    }
    CG_HIP(hipStreamSynchronize(st));
    if (!kept || 5LL * n > 4LL * nf) return CGAMD_OK;
    tmp.keep(agg, h); tmp.keep(mem, h); tmp.keep(kp, h); tmp.keep(kc, h); tmp.keep(kv, h);
    F.agg = static_cast<const int *>(agg);
    F.mem = static_cast<const int *>(mem);
    C->n = C->nu = n;
    C->nnz = nnz;
    C->vals = kv; C->ptr = static_cast<const int *>(kp); C->cols = static_cast<const int *>(kc);
    *built = true;
    return CGAMD_OK;
}

// the coefficients of every system of a level, in double from its own bound, and their table on the device, rounded to the real type
static int batched_coefficients(MgHierarchy *h, MgLevel &L, double kappa, hipStream_t st) {
    const size_t ns = (size_t)h->nsys, steps = (size_t)L.steps;
    const bool dbl = h->dtype == CGAMD_F64 || h->dtype == CGAMD_C128;
    const size_t rs = dbl ? 8 : 4;
    L.c0.assign(steps * ns, 0.);
    L.c1.assign(steps * ns, 0.);
    std::vector<double> a, b;
    for (size_t r = 0; r < ns; ++r) {
        cheb_coefficients(L.lmaxs[r], kappa, L.steps, &a, &b);
        for (size_t k = 0; k < steps; ++k) { L.c0[k * ns + r] = a[k]; L.c1[k * ns + r] = b[k]; }
    }
    std::vector<double> td(2 * steps * ns);
    std::vector<float> tf(dbl ? 0 : 2 * steps * ns);
    for (size_t k = 0; k < steps; ++k)
        for (size_t r = 0; r < ns; ++r) {
            td[2 * k * ns + r] = L.c0[k * ns + r];
            td[(2 * k + 1) * ns + r] = L.c1[k * ns + r];
        }
    for (size_t i = 0; i < tf.size(); ++i) tf[i] = (float)td[i];
    if (int rc = h->get(&L.coef, 2 * steps * ns * rs, "smoother coefficients")) return rc;
    CG_HIP(hipMemcpyAsync(L.coef, dbl ? static_cast<const void *>(td.data()) : static_cast<const void *>(tf.data()), 2 * steps * ns * rs,
                          hipMemcpyHostToDevice, st));
    CG_HIP(hipStreamSynchronize(st));       // (the host table goes out of scope)
    return CGAMD_OK;
}

int mg_build(hipStream_t st, int dt, int nu, int n, int nrhs, int nsys, const SpmvPlan &plan0, long long nnz, const void *vals,
             const int *ptr, const int *cols, const MgParams &p, const std::string &who, MgHierarchy **out) {
    *out = nullptr;
    const size_t vs = dtype_size(dt);
    const int E = (int)(16 / vs);
    MgHierarchy *h = new MgHierarchy;
    struct Guard { MgHierarchy *h; ~Guard() { delete h; } } guard{h};
    h->dtype = dt; h->nrhs = nrhs; h->nsys = nsys; h->p = p;
    if (nsys && (p.algebraic || nrhs != nsys)) return fail(CGAMD_ERR_STATE, who + ": a batched hierarchy is a grid hierarchy with one right-hand side per system");
    const size_t nmat = nsys ? (size_t)nsys : 1;      // value arrays of a level
    void *words = nullptr;      // [0] error word / Gershgorin bits, [1] scan overflow flag, [2..] scratch of compute_spmv_plan
    if (int rc = h->get(&words, 64, "setup words")) return rc;
    unsigned long long *word = static_cast<unsigned long long *>(words);
    int *flag = reinterpret_cast<int *>(word + 1), *scratch = reinterpret_cast<int *>(word + 2);

    MgLevel L0;
    L0.n = n; L0.nu = nu; L0.nnz = nnz; L0.ld = n;
    L0.grid.nx = p.nx; L0.grid.ny = p.ny; L0.grid.nz = p.nz;
    L0.vals = vals; L0.ptr = ptr; L0.cols = cols; L0.plan = plan0;
    h->lv.push_back(L0);
    if (int rc = level_diagonal(h, h->lv[0], 0, word, who, st)) return rc;

    while (!p.algebraic && h->lv.back().nu > p.min_rows && (int)h->lv.size() < kMgMaxLevels) {
        const int level = (int)h->lv.size();
        MgGrid &g = h->lv.back().grid;
        g.cnx = (g.nx + 1) / 2; g.cny = (g.ny + 1) / 2; g.cnz = (g.nz + 1) / 2;
        const long long ncl = (long long)g.cnx * g.cny * g.cnz;
        if (ncl >= h->lv.back().nu) break;      // (a single node: nothing left to aggregate)
        const int nc = (int)ncl;
        const MgLevel &F = h->lv.back();
        MgLevel C;
        C.n = C.nu = nc;
        C.ld = ((long long)nc + E - 1) / E * E;
        C.grid.nx = g.cnx; C.grid.ny = g.cny; C.grid.nz = g.cnz;
        void *ptrc = nullptr, *colsc = nullptr, *valsc = nullptr;
        if (int rc = h->get(&ptrc, ((size_t)nc + 1 + 64) * 4, "row pointers")) return rc;
        CG_HIP(hipMemsetAsync(word, 0xff, 8, st));
        CG_HIP(hipMemsetAsync(flag, 0, 4, st));
        if (int rc = launch_mg_count(g, nc, F.ptr, F.cols, static_cast<int *>(ptrc), word, st)) return rc;
        if (int rc = launch_mg_scan(nc, static_cast<int *>(ptrc), flag, st)) return rc;
        unsigned long long err_h = 0;
        int back[2] = {0, 0};     // overflow flag, coarse nnz
        CG_HIP(hipMemcpyAsync(&err_h, word, 8, hipMemcpyDeviceToHost, st));
        CG_HIP(hipMemcpyAsync(&back[0], flag, 4, hipMemcpyDeviceToHost, st));
        CG_HIP(hipMemcpyAsync(&back[1], static_cast<int *>(ptrc) + nc, 4, hipMemcpyDeviceToHost, st));
        CG_HIP(hipStreamSynchronize(st));
        if (err_h != ~0ull)
            return fail(CGAMD_ERR_INVALID, who + ": level " + std::to_string(level) + ": coarse row " + std::to_string(err_h) + " has more than " +
                                               std::to_string(kMgMaxRow) + " distinct columns");
        if (back[0]) return fail(CGAMD_ERR_INVALID, who + ": level " + std::to_string(level) + ": the coarse matrix has more than 2^31 - 1 entries");
        C.nnz = back[1];
        // (64 entries of zeroed padding behind both arrays, as the handle's own matrix carries for the row-block kernels)
        if (int rc = h->get(&colsc, ((size_t)C.nnz + 64) * 4, "columns")) return rc;
        if (int rc = h->get(&valsc, ((size_t)C.nnz * nmat + 64) * vs, "values")) return rc;
        CG_HIP(hipMemsetAsync(colsc, 0, ((size_t)C.nnz + 64) * 4, st));
        CG_HIP(hipMemsetAsync(valsc, 0, ((size_t)C.nnz * nmat + 64) * vs, st));
        if (nsys) {
            if (int rc = launch_mg_fill_batched(dt, g, nc, nsys, F.nnz, C.nnz, F.vals, F.ptr, F.cols, static_cast<int *>(ptrc),
                                                static_cast<int *>(colsc), valsc, st)) return rc;
        } else if (int rc = launch_mg_fill(dt, g, nc, F.vals, F.ptr, F.cols, static_cast<int *>(ptrc), static_cast<int *>(colsc), valsc, st)) return rc;
        C.vals = valsc; C.ptr = static_cast<int *>(ptrc); C.cols = static_cast<int *>(colsc);
        C.plan = make_spmv_plan(nc);
        if (int rc = compute_spmv_plan(C.ptr, C.cols, nc, scratch, st, &C.plan)) return rc;
        finalize_spmv_plan(&C.plan, dt, nrhs, nc, C.nnz, C.vals, C.cols);
        if (nsys) batched_level_plan(&C.plan, dt, nsys, nc, C.nnz);
        h->lv.push_back(C);
        if (int rc = level_diagonal(h, h->lv.back(), level, word, who, st)) return rc;
    }
    while (p.algebraic && h->lv.back().nu > p.min_rows && (int)h->lv.size() < kMgMaxLevels) {
        const int level = (int)h->lv.size();
        MgLevel C;
        bool built = false;
        if (int rc = amg_coarsen(h, word, flag, who, st, &C, &built)) return rc;
        if (!built) break;
        const int nc = C.nu;
        C.ld = ((long long)nc + E - 1) / E * E;
        C.plan = make_spmv_plan(nc);
        if (int rc = compute_spmv_plan(C.ptr, C.cols, nc, scratch, st, &C.plan)) return rc;
        finalize_spmv_plan(&C.plan, dt, nrhs, nc, C.nnz, C.vals, C.cols);
        h->lv.push_back(C);
        if (int rc = level_diagonal(h, h->lv.back(), level, word, who, st)) return rc;
    }

    const int nl = (int)h->lv.size();
    for (int l = 0; l < nl; ++l) {
        MgLevel &L = h->lv[(size_t)l];
        const bool coarsest = l == nl - 1;
        L.steps = coarsest ? kMgCoarsestSteps : p.smooth_steps;
        if (nsys) {
            if (int rc = batched_coefficients(h, L, coarsest ? kMgKappaCoarsest : kMgKappaSmooth, st)) return rc;
        } else cheb_coefficients(L.lmax, coarsest ? kMgKappaCoarsest : kMgKappaSmooth, L.steps, &L.c0, &L.c1);
        const size_t bytes = (size_t)L.ld * (size_t)nrhs * vs;
        if (int rc = h->get(&L.w, bytes, "w")) return rc;
        CG_HIP(hipMemsetAsync(L.w, 0, bytes, st));
        if (L.steps > 1) {
            if (int rc = h->get(&L.d, bytes, "d")) return rc;
            CG_HIP(hipMemsetAsync(L.d, 0, bytes, st));
        }
        if (l > 0) {
            if (int rc = h->get(&L.x, bytes, "x")) return rc;
            if (int rc = h->get(&L.b, bytes, "b")) return rc;
            CG_HIP(hipMemsetAsync(L.x, 0, bytes, st));
            CG_HIP(hipMemsetAsync(L.b, 0, bytes, st));
        }
    }
    CG_HIP(hipStreamSynchronize(st));
    guard.h = nullptr;
    *out = h;
    return CGAMD_OK;
}

void mg_free(MgHierarchy *h) { delete h; }

// The V-cycle, walked once for the launches (st) or once for the tally (cost != nullptr: nothing is launched)
static int mg_walk(const MgHierarchy *h, const void *r, void *z, hipStream_t st, MgCost *cost) {
    const int dt = h->dtype, nr = h->nrhs, nl = (int)h->lv.size();
    const long long V = (long long)dtype_size(dt);
    const int ns = h->nsys;
    const long long nm = ns ? ns : 1;                   // value arrays and dinv arrays of a level: one per system of a batched hierarchy
    const size_t rs = (dt == CGAMD_F64 || dt == CGAMD_C128) ? 8 : 4;
    auto vec = [&](const MgLevel &L, int passes, int shared) {       // passes over nrhs-wide vectors, shared = over dinv
        if (cost) { ++cost->launches; cost->bytes += ((long long)passes * nr + shared * nm) * L.n * V; }
    };
    auto spmv = [&](const MgLevel &L, int l, const void *x, void *w) -> int {
        if (cost) {
            ++cost->launches;
            if (l == 0) ++cost->spmv0;
            else cost->bytes += L.nnz * (nm * V + 4) + ((long long)L.n + 1) * 4 + 2LL * L.n * V * nr;
            return CGAMD_OK;
        }
        if (ns) return launch_spmv_batched(dt, L.plan, L.n, L.nnz, ns, L.vals, L.ptr, L.cols, x, L.ld, w, L.ld, nullptr, nullptr, st);
        return launch_spmv(dt, L.plan, L.n, L.nnz, L.vals, L.ptr, L.cols, x, L.ld, w, L.ld, nr, nullptr, nullptr, st);
    };
    auto later_steps = [&](const MgLevel &L, int l, const void *b, void *x) -> int {       // steps 1 .. steps - 1 of a smoothing
        for (int k = 1; k < L.steps; ++k) {
            if (int rc = spmv(L, l, x, L.w)) return rc;
            vec(L, 7, 1);
            if (!cost && ns) {
                if (int rc = launch_mg_cheb_batched(dt, 2, L.n, L.ld, ns, L.dinv, b, L.w, L.d, x, L.coef0(k, ns, rs), L.coef1(k, ns, rs), true, st)) return rc;
            } else if (!cost)
                if (int rc = launch_mg_cheb(dt, 2, L.n, L.ld, nr, L.dinv, b, L.w, L.d, x, L.c0[(size_t)k], L.c1[(size_t)k], true, st)) return rc;
        }
        return CGAMD_OK;
    };
    for (int l = 0; l < nl; ++l) {
        const MgLevel &L = h->lv[(size_t)l];
        const void *b = l == 0 ? r : L.b;
        void *x = l == 0 ? z : L.x;
        if (l == 0) {       // (the first step of every coarse level rides in the restriction that makes its b)
            vec(L, 2 + (L.steps > 1), 1);
            if (!cost && ns) {
                if (int rc = launch_mg_cheb_batched(dt, 0, L.n, L.ld, ns, L.dinv, b, nullptr, L.d, x, nullptr, L.coef1(0, ns, rs), L.steps > 1, st)) return rc;
            } else if (!cost)
                if (int rc = launch_mg_cheb(dt, 0, L.n, L.ld, nr, L.dinv, b, nullptr, L.d, x, 0., L.c1[0], L.steps > 1, st)) return rc;
        }
        if (int rc = later_steps(L, l, b, x)) return rc;
        if (l == nl - 1) break;
        const MgLevel &C = h->lv[(size_t)l + 1];
        if (int rc = spmv(L, l, x, L.w)) return rc;
        if (cost) { ++cost->launches; cost->bytes += 2LL * nr * L.nu * V + ((2LL + (C.steps > 1)) * nr + nm) * C.n * V + (L.mem ? 4LL * kAmgWidth * C.n : 0); }
        else if (ns) {
            if (int rc = launch_mg_restrict_batched(dt, L.grid, C.nu, L.ld, C.ld, ns, b, L.w, C.b, C.dinv, C.x, C.d, C.coef1(0, ns, rs), C.steps > 1, st)) return rc;
        } else if (L.mem) {
            if (int rc = launch_amg_restrict(dt, C.nu, L.mem, L.ld, C.ld, nr, b, L.w, C.b, C.dinv, C.x, C.d, C.c1[0], C.steps > 1, st)) return rc;
        } else if (int rc = launch_mg_restrict(dt, L.grid, C.nu, L.ld, C.ld, nr, b, L.w, C.b, C.dinv, C.x, C.d, C.c1[0], C.steps > 1, st)) return rc;
    }
    for (int l = nl - 2; l >= 0; --l) {
        const MgLevel &L = h->lv[(size_t)l], &C = h->lv[(size_t)l + 1];
        const void *b = l == 0 ? r : L.b;
        void *x = l == 0 ? z : L.x;
        if (cost) { ++cost->launches; cost->bytes += 2LL * nr * L.nu * V + (long long)nr * C.n * V + (L.agg ? 4LL * L.nu : 0); }
        else if (L.agg) {
            if (int rc = launch_amg_prolong(dt, L.nu, L.agg, L.ld, C.ld, nr, C.x, x, h->p.omega, st)) return rc;
        } else if (int rc = launch_mg_prolong(dt, L.grid, L.nu, L.ld, C.ld, nr, C.x, x, h->p.omega, st)) return rc;
        if (int rc = spmv(L, l, x, L.w)) return rc;
        vec(L, 4 + (L.steps > 1), 1);
        if (!cost && ns) {
            if (int rc = launch_mg_cheb_batched(dt, 1, L.n, L.ld, ns, L.dinv, b, L.w, L.d, x, nullptr, L.coef1(0, ns, rs), L.steps > 1, st)) return rc;
        } else if (!cost)
            if (int rc = launch_mg_cheb(dt, 1, L.n, L.ld, nr, L.dinv, b, L.w, L.d, x, 0., L.c1[0], L.steps > 1, st)) return rc;
        if (int rc = later_steps(L, l, b, x)) return rc;
    }
    return CGAMD_OK;
}

int mg_vcycle(const MgHierarchy *h, const void *r, void *z, hipStream_t st) { return mg_walk(h, r, z, st, nullptr); }
MgCost mg_cost(const MgHierarchy *h) {
    MgCost c;
    (void)mg_walk(h, nullptr, nullptr, nullptr, &c);
    return c;
}
int mg_levels(const MgHierarchy *h) { return (int)h->lv.size(); }
int mg_level_info(const MgHierarchy *h, int level, long long info[6]) {
    if (level < 0 || level >= (int)h->lv.size()) return fail(CGAMD_ERR_INVALID, "mg_level: no such level");
    const MgLevel &L = h->lv[(size_t)level];
    info[0] = L.nu; info[1] = L.nnz; info[2] = L.grid.nx; info[3] = L.grid.ny; info[4] = L.grid.nz;
    if (h->p.algebraic) { info[2] = L.nu; info[3] = info[4] = 0; }
    std::memcpy(&info[5], &L.lmax, 8);
    return CGAMD_OK;
}
int mg_level_bounds(const MgHierarchy *h, int level, double *lmax, int count) {
    if (level < 0 || level >= (int)h->lv.size()) return fail(CGAMD_ERR_INVALID, "mg_level_bounds: no such level");
    if (!lmax || count < 0 || count > (h->nsys ? h->nsys : 1)) return fail(CGAMD_ERR_INVALID, "mg_level_bounds: count is 0 ... the systems of the hierarchy (1 on a single-system handle)");
    const MgLevel &L = h->lv[(size_t)level];
    for (int r = 0; r < count; ++r) lmax[r] = h->nsys ? L.lmaxs[(size_t)r] : L.lmax;
    return CGAMD_OK;
}
int mg_level_matrix(const MgHierarchy *h, int level, int *ptr, int *cols, void *vals, hipStream_t st) {
    if (level < 0 || level >= (int)h->lv.size()) return fail(CGAMD_ERR_INVALID, "mg_level_matrix: no such level");
    const MgLevel &L = h->lv[(size_t)level];
    if (ptr) CG_HIP(hipMemcpyAsync(ptr, L.ptr, ((size_t)L.nu + 1) * 4, hipMemcpyDeviceToHost, st));
    if (cols) CG_HIP(hipMemcpyAsync(cols, L.cols, (size_t)L.nnz * 4, hipMemcpyDeviceToHost, st));
    if (vals) CG_HIP(hipMemcpyAsync(vals, L.vals, (size_t)L.nnz * (h->nsys ? (size_t)h->nsys : 1) * dtype_size(h->dtype), hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    return CGAMD_OK;
}
int mg_aggregates(const MgHierarchy *h, int level, int *agg_host, int *n_coarse, hipStream_t st) {
    if (level < 0 || level + 1 >= (int)h->lv.size()) return fail(CGAMD_ERR_INVALID, "mg_aggregates: no level below this one");
    const MgLevel &L = h->lv[(size_t)level];
    if (n_coarse) *n_coarse = h->lv[(size_t)level + 1].nu;
    if (!agg_host) return CGAMD_OK;
    if (L.agg) {
        CG_HIP(hipMemcpyAsync(agg_host, L.agg, (size_t)L.nu * 4, hipMemcpyDeviceToHost, st));
        CG_HIP(hipStreamSynchronize(st));
        return CGAMD_OK;
    }
    const MgGrid &g = L.grid;       // the box map, as mg_agg computes it
    for (int i = 0; i < L.nu; ++i) {
        const int x = i % g.nx, t = i / g.nx, y = t % g.ny, z = t / g.ny;
        agg_host[i] = (x >> 1) + g.cnx * ((y >> 1) + g.cny * (z >> 1));
    }
    return CGAMD_OK;
}

// ---- development entries (tests): what a level holds, and one level's product as the cycle launches it ----------------------------
int mg_level_state(const MgHierarchy *h, int level, int which, void *out_host, long long cap_values, long long *count, hipStream_t st) {
    if (level < 0 || level >= (int)h->lv.size()) return fail(CGAMD_ERR_INVALID, "mg_level_state: no such level");
    const MgLevel &L = h->lv[(size_t)level];
    int five[5] = {L.n, L.nu, (int)L.ld, L.steps, h->p.algebraic ? 1 : 0};
    const void *host = nullptr, *dev = nullptr;
    size_t each = 0;
    long long values = 0;
    switch (which) {
    case 0: host = five; each = sizeof(int); values = 5; break;
    case 1: dev = L.dinv; each = dtype_size(h->dtype); values = h->nsys ? L.ld * h->nsys : L.n; break;
    case 2: host = L.c0.data(); each = sizeof(double); values = (long long)L.c0.size(); break;
    case 3: host = L.c1.data(); each = sizeof(double); values = (long long)L.c1.size(); break;
    case 4:
        if (!L.mem || level + 1 >= (int)h->lv.size())
            return fail(CGAMD_ERR_INVALID, "mg_level_state: the level has no member lists (a grid hierarchy, or the coarsest level)");
        dev = L.mem; each = sizeof(int); values = (long long)kAmgWidth * h->lv[(size_t)level + 1].nu;
        break;
    default: return fail(CGAMD_ERR_INVALID, "mg_level_state: which is 0 .. 4");
    }
    *count = values;
    if (cap_values < values) return fail(CGAMD_ERR_INVALID, "mg_level_state: output holds fewer values than the state has");
    if (host) std::memcpy(out_host, host, each * (size_t)values);
    else CG_HIP(hipMemcpyAsync(out_host, dev, each * (size_t)values, hipMemcpyDeviceToHost, st));
    CG_HIP(hipStreamSynchronize(st));
    return CGAMD_OK;
}
// one V-cycle on caller vectors (nrhs * n_user device values each, stride n_user), through buffers with the handle's padding rows
// (n >= n_user rows, the padding zero); synchronises
int mg_apply_padded(MgHierarchy *h, hipStream_t st, int dtype, int n, int n_user, int nrhs, const void *r_dev, void *z_dev, const char *who) {
    const size_t vs = dtype_size(dtype), row = (size_t)n * vs, user = (size_t)n_user * vs, bytes = row * (size_t)nrhs;
    void *buf = nullptr;
    if (int rc = dmalloc(&buf, 2 * bytes, "mg_apply vectors")) return rc;
    void *r = buf, *z = static_cast<char *>(buf) + bytes;
    int rc = CGAMD_OK;
    hipError_t e = hipMemsetAsync(buf, 0, 2 * bytes, st);
    if (e == hipSuccess) e = hipMemcpy2DAsync(r, row, r_dev, user, user, (size_t)nrhs, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) rc = mg_vcycle(h, r, z, st);
    if (e == hipSuccess && !rc) e = hipMemcpy2DAsync(z_dev, user, z, row, user, (size_t)nrhs, hipMemcpyDeviceToDevice, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(buf);
    if (rc) return rc;
    if (e != hipSuccess || e2 != hipSuccess) return fail(CGAMD_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e != hipSuccess ? e : e2));
    return CGAMD_OK;
}
int mg_level_spmv(const MgHierarchy *h, int level, const void *x, void *w, hipStream_t st) {
    if (level < 0 || level >= (int)h->lv.size()) return fail(CGAMD_ERR_INVALID, "mg_level_spmv: no such level");
    const MgLevel &L = h->lv[(size_t)level];
    if (h->nsys) {
        if (int rc = launch_spmv_batched(h->dtype, L.plan, L.n, L.nnz, h->nsys, L.vals, L.ptr, L.cols, x, L.ld, w, L.ld, nullptr, nullptr, st)) return rc;
    } else if (int rc = launch_spmv(h->dtype, L.plan, L.n, L.nnz, L.vals, L.ptr, L.cols, x, L.ld, w, L.ld, h->nrhs, nullptr, nullptr, st)) return rc;
    CG_HIP(hipStreamSynchronize(st));
    return CGAMD_OK;
}

}  // namespace cgamd

// ---- the cycle kernels and the scan as stateless entries (include/cgamd.h "Multigrid: the kernels"): thin wrappers over the launch_*
// the cycle and the setup call, with pointers and leading dimensions left to the caller.  What can be judged without a device is
// judged first, the context last.
using namespace cgamd;

static int mg_op(cgamd_ctx *ctx, int dtype, const char *what) {
    if (dtype < 0 || dtype > 3) return fail(CGAMD_ERR_INVALID, std::string(what) + ": dtype must be one of the four value types");
    if (!ctx) return fail(CGAMD_ERR_INVALID, std::string(what) + ": ctx is NULL");
    thread_hip_setup();
    CG_HIP(hipSetDevice(ctx->device));
    return CGAMD_OK;
}
static int mg_done(cgamd_ctx *ctx, int rc) {
    if (rc) return rc;
    CG_HIP(hipStreamSynchronize(ctx->stream));
    return CGAMD_OK;
}
// the grid of a box map; false when a dimension is below 1 or the rows do not fit an int
static bool mg_box(int nx, int ny, int nz, MgGrid *g, long long *nf, long long *nc) {
    if (nx < 1 || ny < 1 || nz < 1) return false;
    g->nx = nx; g->ny = ny; g->nz = nz;
    g->cnx = (nx + 1) / 2; g->cny = (ny + 1) / 2; g->cnz = (nz + 1) / 2;
    *nf = (long long)nx * ny * nz;
    *nc = (long long)g->cnx * g->cny * g->cnz;
    return *nf <= 2147483647LL;
}

extern "C" {

int cgamd_mg_smooth_step(cgamd_ctx *ctx, int dtype, int mode, int size, long long ld, int nRHS, const void *dinv, const void *b, const void *w,
                         void *d, void *x, double c0, double c1, int store_d) {
    if (mode < 0 || mode > 2) return fail(CGAMD_ERR_INVALID, "mg_smooth_step: mode is 0, 1 or 2");
    if (!dinv || !b || !x || (mode != 0 && !w) || ((mode == 2 || store_d) && !d)) return fail(CGAMD_ERR_INVALID, "mg_smooth_step: null pointer");
    if (size < 0 || nRHS < 1) return fail(CGAMD_ERR_INVALID, "mg_smooth_step: bad size/nRHS");
    if (ld < size) return fail(CGAMD_ERR_INVALID, "mg_smooth_step: leading dimension below size");
    if (int rc = mg_op(ctx, dtype, "mg_smooth_step")) return rc;
    return mg_done(ctx, launch_mg_cheb(dtype, mode, size, ld, nRHS, dinv, b, w, d, x, c0, c1, store_d != 0, ctx->stream));
}

int cgamd_mg_restrict(cgamd_ctx *ctx, int dtype, int nx, int ny, int nz, const int *members, int n_coarse, long long ld_f, long long ld_c,
                      int nRHS, const void *b, const void *w, void *bc, const void *dinv_c, void *xc, void *dc, double c1, int store_d) {
    if (!b || !w || !bc || !dinv_c || !xc || (store_d && !dc)) return fail(CGAMD_ERR_INVALID, "mg_restrict: null pointer");
    if (n_coarse < 0 || nRHS < 1) return fail(CGAMD_ERR_INVALID, "mg_restrict: bad size/nRHS");
    MgGrid g;
    long long nf = nx, nc = n_coarse;
    if (members ? nx < 1 : !mg_box(nx, ny, nz, &g, &nf, &nc)) return fail(CGAMD_ERR_INVALID, "mg_restrict: bad size/nRHS");
    if (nc != n_coarse) return fail(CGAMD_ERR_INVALID, "mg_restrict: n_coarse is not the number of boxes of the grid");
    if (ld_f < nf || ld_c < n_coarse) return fail(CGAMD_ERR_INVALID, "mg_restrict: leading dimension below size");
    if (int rc = mg_op(ctx, dtype, "mg_restrict")) return rc;
    if (n_coarse == 0) return CGAMD_OK;
    if (members) return mg_done(ctx, launch_amg_restrict(dtype, n_coarse, members, ld_f, ld_c, nRHS, b, w, bc, dinv_c, xc, dc, c1, store_d != 0, ctx->stream));
    return mg_done(ctx, launch_mg_restrict(dtype, g, n_coarse, ld_f, ld_c, nRHS, b, w, bc, dinv_c, xc, dc, c1, store_d != 0, ctx->stream));
}

int cgamd_mg_prolong(cgamd_ctx *ctx, int dtype, int nx, int ny, int nz, const int *agg, int n_fine, long long ld_f, long long ld_c, int nRHS,
                     const void *e, void *x, double omega) {
    if (!e || !x) return fail(CGAMD_ERR_INVALID, "mg_prolong: null pointer");
    if (n_fine < 0 || nRHS < 1) return fail(CGAMD_ERR_INVALID, "mg_prolong: bad size/nRHS");
    MgGrid g;
    long long nf = n_fine, nc = 1;
    if (!agg && (!mg_box(nx, ny, nz, &g, &nf, &nc) || n_fine > nf)) return fail(CGAMD_ERR_INVALID, "mg_prolong: bad size/nRHS");
    if (ld_f < n_fine || ld_c < nc) return fail(CGAMD_ERR_INVALID, "mg_prolong: leading dimension below size");
    if (int rc = mg_op(ctx, dtype, "mg_prolong")) return rc;
    if (n_fine == 0) return CGAMD_OK;
    if (agg) return mg_done(ctx, launch_amg_prolong(dtype, n_fine, agg, ld_f, ld_c, nRHS, e, x, omega, ctx->stream));
    return mg_done(ctx, launch_mg_prolong(dtype, g, n_fine, ld_f, ld_c, nRHS, e, x, omega, ctx->stream));
}

int cgamd_mg_scan(cgamd_ctx *ctx, int n, int *counts_to_ptr, int *overflow) {
    if (!counts_to_ptr || !overflow) return fail(CGAMD_ERR_INVALID, "mg_scan: null pointer");
    if (n < 0) return fail(CGAMD_ERR_INVALID, "mg_scan: bad size");
    if (int rc = mg_op(ctx, CGAMD_F64, "mg_scan")) return rc;
    return mg_done(ctx, launch_mg_scan(n, counts_to_ptr, overflow, ctx->stream));
}

}  // extern "C"
