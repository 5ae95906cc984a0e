// What a multigrid hierarchy is built with, and the range checks of the entries that take it from a caller (mg_params.cpp).  No HIP
// header: the checks are host code that their CPU test compiles into a program of its own.  Included by cgamd_internal.h.
#pragma once
#include <string>

namespace cgamd {

int fail(int status, const std::string &msg);

// algebraic: aggregates by `passes` passes of matching at strength `theta` (cgamd_solver_set_preconditioner_amg), nx, ny, nz unused
struct MgParams { int nx = 1, ny = 1, nz = 1, smooth_steps = 1, min_rows = 512; double omega = 1.6; bool algebraic = false; int passes = 3; double theta = 0.25; };

// The argument checks of cgamd_solver_set_preconditioner_multigrid, _batched_multigrid and cgamd_dist_set_preconditioner_multigrid
// (`rows`: the rows the box must hold; rows_note: what the entry appends to that refusal) and of the two _amg entries, in the order
// the entries have always made them.  *out <- the defaults, with every argument that is not 0 in its place.  `who` heads each message.
int mg_params_grid(const std::string &who, long long rows, const char *rows_note, int nx, int ny, int nz, int smooth_steps,
                   double over_correction, int min_rows, MgParams *out);
int mg_params_amg(const std::string &who, int passes, double strength, int smooth_steps, double over_correction, int min_rows, MgParams *out);

}  // namespace cgamd
