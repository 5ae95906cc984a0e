// The range checks of the multigrid and AMG preconditioner entries of every handle type (solver_precond.cpp, dist.cpp): one copy of
// each rule, its status and its text.  Host code without a HIP header (tests/mg_params_main.cpp links this file alone).
#include <cmath>

#include "../../include/cgamd.h"
#include "mg_params.h"

namespace cgamd {

// the options the grid and the algebraic form share, checked in this order behind the form's own arguments
static int cycle_options(const std::string &who, int smooth_steps, double over_correction, int min_rows, MgParams *p) {
    if (smooth_steps < 0 || smooth_steps > 4) return fail(CGAMD_ERR_INVALID, who + ": smooth_steps must be in 0 ... 4 (0 = the default, 1)");
    if (!std::isfinite(over_correction) || over_correction < 0.) return fail(CGAMD_ERR_INVALID, who + ": over_correction must be finite and not negative (0 = the default, 1.6)");
    if (min_rows < 0) return fail(CGAMD_ERR_INVALID, who + ": min_rows must not be negative (0 = the default, 512)");
    if (smooth_steps) p->smooth_steps = smooth_steps;
    if (over_correction != 0.) p->omega = over_correction;
    if (min_rows) p->min_rows = min_rows;
    return CGAMD_OK;
}

int mg_params_grid(const std::string &who, long long rows, const char *rows_note, int nx, int ny, int nz, int smooth_steps,
                   double over_correction, int min_rows, MgParams *out) {
    if (nx < 1 || ny < 1 || nz < 1) return fail(CGAMD_ERR_INVALID, who + ": every grid dimension must be at least 1");
    const long long plane = (long long)nx * ny;
    if (plane > 2147483647LL || plane * nz != rows)
        return fail(CGAMD_ERR_INVALID, who + ": nx * ny * nz must equal the size of the system" + (rows_note ? rows_note : ""));
    MgParams p;
    p.nx = nx; p.ny = ny; p.nz = nz;
    if (int rc = cycle_options(who, smooth_steps, over_correction, min_rows, &p)) return rc;
    *out = p;
    return CGAMD_OK;
}

int mg_params_amg(const std::string &who, int passes, double strength, int smooth_steps, double over_correction, int min_rows, MgParams *out) {
    if (passes < 0 || passes > 3) return fail(CGAMD_ERR_INVALID, who + ": passes must be in 0 ... 3 (0 = the default, 3)");
    if (!std::isfinite(strength) || strength < 0. || strength > 1.) return fail(CGAMD_ERR_INVALID, who + ": strength must be in (0, 1] (0 = the default, 0.25)");
    MgParams p;
    p.algebraic = true;
    if (passes) p.passes = passes;
    if (strength != 0.) p.theta = strength;
    if (int rc = cycle_options(who, smooth_steps, over_correction, min_rows, &p)) return rc;
    *out = p;
    return CGAMD_OK;
}

}  // namespace cgamd
