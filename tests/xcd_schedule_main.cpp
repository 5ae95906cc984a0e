// Stand-alone driver of build_xcd_schedule (csrc/xcd_schedule.cpp) for tests/test_xcd_schedule.py, which compiles both files with
// -fsanitize=address,undefined and runs the result as a program.  Input, one case per line: supers rows_per_super unit_rows.
// Output per case, one line: grid, the table's length, xcd_schedule_balanced(supers, grid) as 0 / 1, then the table.
#include <cstdio>
#include <vector>

#include "xcd_schedule.h"

int main() {
    int supers, rows_per_super;
    long long unit_rows;
    while (std::scanf("%d %d %lld", &supers, &rows_per_super, &unit_rows) == 3) {
        std::vector<int> table(3, 12345);       // (stale content: the function owns the size)
        const int grid = cgamd::build_xcd_schedule(supers, rows_per_super, unit_rows, table);
        table.shrink_to_fit();                  // exactly as long as the function made it: a read past its end is a sanitizer finding
        std::printf("%d %zu %d", grid, table.size(), cgamd::xcd_schedule_balanced(supers, grid) ? 1 : 0);
        for (int b = 0; b < grid; ++b) std::printf(" %d", table.data()[b]);
        std::printf("\n");
    }
    return 0;
}
