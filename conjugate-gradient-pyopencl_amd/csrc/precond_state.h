// The preconditioner in force on a handle -- single, batched (cgamd_solver) or row-partitioned (cgamd_dist): what M is, what it was
// built from, and the device memory that belongs to it.  One owner: the handles install, replace and remove M through the functions
// below and read the fields; the loops' own partial buffers (part_rz, part_pcg) and everything about graphs stay on the handles.
#pragma once
#include "cgamd_internal.h"

namespace cgamd {

struct Precond {
    // the form of M, which decides the loop: none, z = m .* r, the line sweeps, a V-cycle
    enum Kind { kNone, kDiag, kTri, kMg };
    // where M came from = what a refresh / reload of the matrix builds again; kCaller (the caller's arrays): nothing
    enum Built { kCaller, kJacobi, kLine, kGridMg, kAmg };
    Kind kind = kNone;
    Built built = kCaller;
    int route = 0;                      // kLine: TriBuilt::source (2 = factored on the device, 3 = by the host route), else 0
    int stride = 0;                     // kLine: the stride asked for
    void *mdiag = nullptr;              // kDiag: n values (a batched handle: nsys diagonals at stride n)
    TriLaunch tri;                      // kTri: the factors behind tri_coef, the plan behind tri_plan, tri.maps (owned too)
    void *tri_coef = nullptr;
    int *tri_plan = nullptr;
    void *tri_part = nullptr;           // kTri: r.z / r.r partials of the sweeps, [2][nrhs][tri.grid] accumulators
    MgHierarchy *mg = nullptr;          // kMg, with what it was built with
    MgParams mg_params;
    void *rho2 = nullptr;               // parity buffer of rho = r.z, 2 x nrhs values: kept across drops
};

// frees M and tri_part, keeps rho2 (the handle frees it with its own buffers); back to kNone / kCaller
void precond_drop(Precond *p);
int precond_ensure_rho(Precond *p, int dtype, int nrhs);
// The ways M changes: the old M goes and the new one stands.  What is handed in belongs to *p from the call on.
// b: a factored tridiagonal M (nsys > 0: the factors of every system of a batched handle, b->pitch apart); line_stride > 0: the lines
// of the matrix at that stride (kLine), 0: the caller's arrays.  The call allocates the sweeps' partials, the chunk maps of the long
// form and rho2, and where that fails frees b and leaves *p as it was.  It holds the only copy of the sweep-grid rule and of the
// TriLaunch fill.  The other two cannot fail: rho2 is the caller's to ensure first
int precond_take_tri(Precond *p, TriBuilt *b, int dtype, int nrhs, int nsys, int line_stride);
void precond_take_diag(Precond *p, void *m_owned, Precond::Built built);
void precond_take_mg(Precond *p, MgHierarchy *h, const MgParams &params);       // kAmg or kGridMg by params.algebraic

// the r.z and r.r partials of a preconditioned loop: the two halves of one allocation, [nrhs][P] accumulators each
struct PcgPartials { void *rz, *rr; };
inline PcgPartials pcg_partials(void *part, int dtype, int P, int nrhs) {
    return {part, static_cast<char *>(part) + acc_size(dtype) * (size_t)P * nrhs};
}

}  // namespace cgamd
