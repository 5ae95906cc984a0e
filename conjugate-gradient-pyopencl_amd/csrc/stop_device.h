// Device side of cgamd_solver_iterate_until: the per-right-hand-side stop of the launched loops.
//
// A right-hand side r stops in the first iteration whose r.r fails  sqrt|r.r| >= tol[r]  (NaN fails it).  The decision is taken
// where r.r becomes known: in the launch that sums its partials (aypx_beta_x, pcg_aypx_beta), by work-group (0, r), from the very
// value it writes into the history.  The test is evaluated in fp64 whatever the value type (|.| of a complex value: hypot).
//
// Two words per right-hand side keep the exit condition of every launch out of reach of a store of the SAME launch:
//   stop[r]   the stopping iteration, written by the beta launch; the alpha step (cg_alpha, cg_alpha2, the prologue of
//             axpy_dot_alpha), the r update and the sweeps of LATER iterations leave on it.  The beta launch of the stopping iteration
//             itself never reads it: all its work-groups still owe that iteration its x += alpha d.
//   live[r]   cleared by the alpha step that found stop[r] set, i.e. one iteration later; the beta launch leaves on it.
// Every exit is uniform over the work-group (one word per blockIdx.y), before any barrier.
//
// *iter is advanced by right-hand side 0's alpha step while any right-hand side is active (nactive, decremented by each stop), so a
// frozen right-hand side 0 does not hold the others' history rows back, and launches after the last stop change nothing at all.
// A frozen right-hand side repeats its last history entry in the rows the others go on to fill: the beta prologues read
// history[iter - 1] of their own column only, and a read-back of `iterations_done + 1` rows holds no unwritten value.
//
// cgamd_dist_iterate_until (dist.cpp) is the same scheme with one right-hand side and rr = the GLOBALLY reduced r.r, which every rank
// holds bit for bit.  There an exit never sits in front of a mailbox store, a spin, an epoch update or an RCCL call: the kernels that
// carry a reduction round (p2p.hip) finish their share of it first and leave afterwards; the staged and RCCL loops update x before
// the deciding launch, and the d step that follows it leaves on live[] like a beta launch.
#pragma once
#include "cgamd_internal.h"
#include "device_types.h"

namespace cgamd {

CG_DEV double stop_norm(float v) { return sqrt(fabs((double)v)); }
CG_DEV double stop_norm(double v) { return sqrt(fabs(v)); }
CG_DEV double stop_norm(float2 v) { return sqrt(hypot((double)v.x, (double)v.y)); }
CG_DEV double stop_norm(double2 v) { return sqrt(hypot(v.x, v.y)); }

// alpha step, one thread of right-hand side 0: the counter moves while anything is left to iterate
CG_DEV void stop_advance(const CgStop &g, int *iter) {
    if (*g.nactive > 0) *iter = *iter + 1;
}
// alpha step, first thread of the first work-group of a frozen right-hand side
CG_DEV void stop_retire(const CgStop &g, int r) { g.live[r] = 0; }

// beta launch, thread 0 of work-group (0, r) of a right-hand side that ran iteration `it`: rr is the history entry just written
template <typename T> CG_DEV void stop_decide(const CgStop &g, int r, int it, T rr) {
    if (!(stop_norm(rr) >= g.tol[r])) {
        g.stop[r] = it;
        __hip_atomic_fetch_add(g.nactive, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // a count: the order of the stops does not show
    }
}
// beta launch, thread 0 of work-group (0, r) of a frozen right-hand side: row `it` of its history column repeats the row before
// (not in the iteration it stopped in, which launches after the last stop run again)
template <typename T> CG_DEV void stop_repeat_history(const CgStop &g, int r, int it, int nrhs, T *history, int history_cap) {
    if (it > g.stop[r] && it < history_cap) history[(long long)it * nrhs + r] = history[(long long)(it - 1) * nrhs + r];
}

}  // namespace cgamd
