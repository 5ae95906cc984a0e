// Host side of the PLANE-MATCHED schedule of the row- and pair-coded SpMV (xcd_schedule.cpp): which XCD runs which super block (the
// kVcBlocks row blocks one work-group takes).  No HIP in here: the table is compiled into the libraries and, for its CPU test, into a
// stand-alone program.
#pragma once
#include <vector>

namespace cgamd {

constexpr int kXcds = 8;            // work-group b runs on XCD b % 8 as that XCD's (b / 8)-th work-group

// The XCD that runs super block s of rows_per_super rows under a schedule of period unit_rows: floor(8 frac(centre(s) / unit_rows)),
// centre(s) = s rows_per_super + rows_per_super / 2.  Rows r and r + unit_rows -- the neighbours across the handle's largest stride,
// a z plane of a 3-D grid -- then sit on the same XCD (but for the supers that straddle an eighth's edge), whose L2 fetches their
// shared line of x once.
int xcd_of_super(int s, int rows_per_super, long long unit_rows);
// table[b] for b in [0, 8 m): the super block XCD b % 8 runs as its (b / 8)-th work-group, or -1 (padding: that XCD's list is
// shorter than m, the longest).  Every XCD's supers ascend, so each sweeps the matrix front to back, plane by plane, all eight at the
// same pace.  Returns the grid, 8 m; 0 (and an empty table) for arguments that are not positive.
int build_xcd_schedule(int supers, int rows_per_super, long long unit_rows, std::vector<int> &table);
// Whether a table of `grid` work-groups for `supers` super blocks keeps the eight XCDs evenly loaded: a launch lasts as long as the
// longest list, grid / 8, and the formula balances only where the unit drifts against the super blocks.  A unit that is a whole number
// of super blocks but no multiple of 8 (a plane of 9216 rows: 9 blocks) puts two blocks of every plane on the same XCD -- lists of
// 400 / 800, a launch 1.78 times as long.  True where the longest list is at most 2 % above an eighth of the super blocks (the
// measured systems: 0.2 and 0.8 %); the default rule takes the table only then.
bool xcd_schedule_balanced(int supers, int grid);

}  // namespace cgamd
