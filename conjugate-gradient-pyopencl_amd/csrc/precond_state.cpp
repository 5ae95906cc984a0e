// The preconditioner in force on a handle (precond_state.h): install, replace, remove.
#include <algorithm>

#include "precond_state.h"

namespace cgamd {

int dmalloc(void **p, size_t bytes, const char *what) {
    hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess)
        return fail(CGAMD_ERR_ALLOC, std::string("hipMalloc(") + what + ", " + std::to_string(bytes) + " B): " + hipGetErrorString(e));
    return CGAMD_OK;
}

void precond_drop(Precond *p) {
    for (void *q : {p->mdiag, p->tri_coef, (void *)p->tri_plan, p->tri.maps, p->tri_part})
        if (q) (void)hipFree(q);
    if (p->mg) mg_free(p->mg);
    void *rho2 = p->rho2;
    *p = Precond();
    p->rho2 = rho2;
}

int precond_ensure_rho(Precond *p, int dtype, int nrhs) {
    if (p->rho2) return CGAMD_OK;
    return dmalloc(&p->rho2, 2 * dtype_size(dtype) * (size_t)nrhs, "rho");
}

int precond_take_tri(Precond *p, TriBuilt *b, int dtype, int nrhs, int nsys, int line_stride) {
    const size_t vs = dtype_size(dtype);
    // work-groups of the sweeps = partials per right-hand side: a chunk each up to 1024 (precond.hip), or the strided form's own rule
    const int grid = b->stride == 1 ? std::min(b->count, 1024) : tri_strided_grid(b->count);
    void *part = nullptr, *maps = nullptr;
    int rc = dmalloc(&part, 2 * acc_size(dtype) * (size_t)grid * nrhs, "partials_rz/rr (tridiagonal)");
    if (!rc && b->longform) rc = dmalloc(&maps, (size_t)tri_maps_values(b->count, nrhs) * vs, "tridiagonal chunk maps");
    if (!rc) rc = precond_ensure_rho(p, dtype, nrhs);
    if (rc) {
        for (void *q : {part, maps})
            if (q) (void)hipFree(q);
        tri_built_free(b);
        return rc;
    }
    precond_drop(p);
    p->kind = Precond::kTri;
    if (line_stride) { p->built = Precond::kLine; p->route = b->source; p->stride = line_stride; }
    p->tri_coef = b->coef;
    p->tri_plan = b->plan;
    p->tri_part = part;
    char *cb = static_cast<char *>(b->coef);
    const size_t arr = b->pitch * vs * (size_t)std::max(nsys, 1);      // nsys > 0: every array holds the factors of all systems, `pitch` apart
    TriLaunch &t = p->tri;
    t.nl = cb; t.ne = cb + arr; t.w = cb + 2 * arr;
    t.fpitch = nsys ? (long long)b->pitch : 0;
    if (b->stride == 1) {
        t.cstart = b->plan;
        t.nchunks = b->count; t.longform = b->longform;
    } else {
        t.stride = b->stride;
        t.segs = b->plan;
        t.nsegs = b->count;
    }
    t.grid = grid;
    t.maps = maps;
    *b = TriBuilt();
    return CGAMD_OK;
}

void precond_take_diag(Precond *p, void *m_owned, Precond::Built built) {
    precond_drop(p);
    p->kind = Precond::kDiag;
    p->built = built;
    p->mdiag = m_owned;
}

void precond_take_mg(Precond *p, MgHierarchy *h, const MgParams &params) {
    precond_drop(p);
    p->kind = Precond::kMg;
    p->built = params.algebraic ? Precond::kAmg : Precond::kGridMg;
    p->mg = h;
    p->mg_params = params;
}

}  // namespace cgamd
