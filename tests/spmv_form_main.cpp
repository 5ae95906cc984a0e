// Stand-alone driver of csrc/spmv_form.cpp for tests/test_spmv_form.py: one decision per input line, one answer per output line.
//   input:   the kSpmvFormInputs ints of cgamd_solver_spmv_form's `inputs` (call, plan, tuning; pointers as 0 / 1)
//   output:  the ten fields of cgamd_last_spmv_form the launch of that call records, then " | " and what the launch needs beyond them
//            (grid_y depth pair_slots table cycle cap chunk body lds); "none" where nothing is launched (an empty row-block list)
//   argument "names": prints the names of the inputs, one per line, and exits
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "spmv_form.h"

int main(int argc, char **argv) {
    using namespace cgamd;
    if (argc > 1 && !std::strcmp(argv[1], "names")) {
        for (int i = 0; i < kSpmvFormInputs; ++i) std::printf("%s\n", kSpmvFormInputNames[i]);
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int a[kSpmvFormInputs], extra;
        for (int i = 0; i < kSpmvFormInputs; ++i) in >> a[i];
        if (!in || (in >> extra)) {
            std::fprintf(stderr, "bad input line: %s\n", line.c_str());
            return 2;
        }
        SpmvPlan plan;
        Tuning t;
        SpmvCall c;
        spmv_form_unpack(a, &plan, &t, &c);
        int back[kSpmvFormInputs];
        spmv_form_pack(plan, t, c, back);
        if (std::memcmp(a, back, sizeof a)) {
            std::fprintf(stderr, "the inputs do not survive unpack / pack: %s\n", line.c_str());
            return 3;
        }
        const SpmvForm f = choose_spmv_form(plan, t, c);
        if (f.family < 0) {
            std::printf("none\n");
            continue;
        }
        int out[kSpmvFormFields];
        f.record(out);
        for (int i = 0; i < kSpmvFormFields; ++i) std::printf(i ? " %d" : "%d", out[i]);
        std::printf(" | %d %d %d %d %d %d %d %d %zu\n", f.grid_y, f.depth, f.pair_slots, f.table, f.cycle, f.cap, f.chunk, f.body, f.lds);
    }
    return 0;
}
