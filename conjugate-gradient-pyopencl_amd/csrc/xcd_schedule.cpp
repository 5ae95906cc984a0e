// PLANE-MATCHED XCD schedule, host side: deal the super blocks of a row- or pair-coded SpMV to the eight XCDs by their place inside
// the handle's largest stride (xcd_schedule.h).  Plain C++; solver.cpp uploads the table once per handle and pattern.
#include "xcd_schedule.h"

#include <cstddef>

using std::size_t;

namespace cgamd {

int xcd_of_super(int s, int rows_per_super, long long unit_rows) {
    const long long centre = (long long)s * rows_per_super + rows_per_super / 2;
    return (int)(kXcds * (centre % unit_rows) / unit_rows);     // (centre % unit_rows < unit_rows: 0 ... 7)
}

int build_xcd_schedule(int supers, int rows_per_super, long long unit_rows, std::vector<int> &table) {
    table.clear();
    if (supers <= 0 || rows_per_super <= 0 || unit_rows <= 0) return 0;
    int count[kXcds] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < supers; ++s) ++count[xcd_of_super(s, rows_per_super, unit_rows)];
    int m = 0;
    for (int x = 0; x < kXcds; ++x) m = count[x] > m ? count[x] : m;
    table.assign((size_t)kXcds * m, -1);
    int next[kXcds] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < supers; ++s) {              // ascending s: every XCD's list ascends
        const int x = xcd_of_super(s, rows_per_super, unit_rows);
        table[(size_t)kXcds * next[x]++ + x] = s;
    }
    return kXcds * m;
}

bool xcd_schedule_balanced(int supers, int grid) {
    return supers > 0 && grid > 0 && (long long)grid * 100 <= (long long)supers * 102;
}

}  // namespace cgamd
