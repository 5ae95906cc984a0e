// Which SpMV form a call of launch_spmv gets, decided ONCE: the launcher (spmv.hip spmv_impl) launches what choose_spmv_form answers,
// and the accessors and byte models of the solver (solver.cpp loop_form) ask the same function.  The plan, the tuning and
// the rules both sides share: spmv_plan.h.  No HIP in here: the decision is compiled into the libraries and, for
// its CPU test (tests/test_spmv_form.py), into a stand-alone program.
#pragma once
#include "spmv_plan.h"

namespace cgamd {

// everything about ONE call the decision reads that is neither in the plan nor in the tuning
struct SpmvCall {
    int value_bytes = 8, acc_bytes = 8;     // size of a value and of its accumulator
    int n = 0, nrhs = 1;
    bool vec = false;                       // aValues and aCols 16-byte aligned
    bool codes_for = false, vcodes_for = false, rcodes_for = false;     // cols / vals / ptr ARE the arrays the plan's codes were made from
    bool fuse = false;                      // d.q partials asked for
    bool rb_list = false;                   // an explicit row-block list was passed ...
    int rb_count = 0;                       // ... of this many blocks
    bool x16 = false, y16 = false, d16 = false;     // x, y, dvec 16-byte aligned
};

constexpr int kSpmvFormFields = 10;
// family: 0 stream, 1 row-block, 2 vc, 3 vcp, 4 chunked, 5 grouped SpMM, 7 row-pattern codes, 8 row pairs, 9 split long rows
// (6: batched.hip); -1: nothing to launch (an empty row-block list)
struct SpmvForm {
    // the record of cgamd_last_spmv_form, in its order and numbering
    int family = -1, vec = 0, width = 0, ienc = 0, venc = 0, nt = 0, fused = 0, wide = 0, grid = 0, parts = 0;
    // what the launch needs beyond it
    int grid_y = 1;         // second grid dimension (the wide form: one work-group per (row block, right-hand side))
    int depth = 0;          // row- and pair-coded kernels: passes whose gathers are in flight per wave
    int pair_slots = 0;     // pair-coded kernel: slots walked, 7 or 8
    int table = 0;          // the grid is the plane-matched schedule table's (the kernel reads plan.sched)
    int cycle = 0;          // block-cyclic schedule: in row blocks, or in super blocks for families 2, 3, 7 and 8
    int cap = 0;            // LDS slice capacity in entries
    int chunk = 0;          // grouped SpMM: right-hand sides per launch
    int body = 0;           // split long rows: there are regular blocks, launched through the block list by the form of the body plan
    size_t lds = 0;         // dynamic LDS bytes
    void record(int *out) const {
        const int f[kSpmvFormFields] = {family, vec, width, ienc, venc, nt, fused, wide, grid, fused ? parts : 0};
        for (int i = 0; i < kSpmvFormFields; ++i) out[i] = f[i];
    }
};
// the plan the regular blocks of a split handle are launched with (their own spans, no long rows)
SpmvPlan long_rows_body(const SpmvPlan &plan);
SpmvForm choose_spmv_form(const SpmvPlan &plan, const Tuning &t, const SpmvCall &c);

// The decision's inputs as a flat int array (pointers as 0 / 1), for cgamd_solver_spmv_form and the CPU test: kSpmvFormInputs ints
// named kSpmvFormInputNames; spmv_form_unpack restores a plan, tuning and call that choose_spmv_form reads alike
constexpr int kSpmvFormInputs = 62;
extern const char *const kSpmvFormInputNames[kSpmvFormInputs];
void spmv_form_pack(const SpmvPlan &plan, const Tuning &t, const SpmvCall &c, int *out);
void spmv_form_unpack(const int *in, SpmvPlan *plan, Tuning *t, SpmvCall *c);

} // namespace cgamd
