// Stand-alone driver of merge_pair_slots (csrc/row_pairs.cpp) for tests/test_row_pairs_merge.py, which compiles both files with
// -fsanitize=address,undefined and runs the result as a program.  Input, one case per line: len0 off0... len1 off1...
// Output per case: "ok n off0 src00 src10 off1 src01 src11 ..." or "long n".
#include <cstdio>
#include <vector>

#include "row_pairs.h"

int main() {
    int len0;
    while (std::scanf("%d", &len0) == 1) {
        std::vector<int> off0(len0);        // exactly as long as the rows: a read past a row's end is a sanitizer finding
        for (int &o : off0) if (std::scanf("%d", &o) != 1) return 2;
        int len1;
        if (std::scanf("%d", &len1) != 1) return 2;
        std::vector<int> off1(len1);
        for (int &o : off1) if (std::scanf("%d", &o) != 1) return 2;
        cgamd::PairPattern pp;
        if (!cgamd::merge_pair_slots(len0, off0.data(), len1, off1.data(), &pp)) { std::printf("long %d\n", pp.n); continue; }
        std::printf("ok %d", pp.n);
        for (int u = 0; u < pp.n; ++u) std::printf(" %d %d %d", pp.off[u], pp.src0[u], pp.src1[u]);
        std::printf("\n");
    }
    return 0;
}
