// The SpMV form decision (spmv_form.h).  Precedence: split long rows, row pair, row code, joint / vcp / vc, row-block on 16-bit /
// 8-bit codes / aCols, chunked, grouped SpMM, stream.
#include "spmv_form.h"

#include <algorithm>
#include <type_traits>

namespace cgamd {

SpmvPlan long_rows_body(const SpmvPlan &plan) {
    const LongRows &lr = plan.lr;
    SpmvPlan body = plan;
    body.lr = LongRows();
    body.kind = lr.body_kind; body.lpr = lr.body_lpr; body.max_span = lr.body_max_span; body.max_row = lr.body_max_row;
    for (int lv = 0; lv < 5; ++lv) body.chunk_span[lv] = lr.body_chunk_span[lv];
    return body;
}

// LDS of a staged slice of `cap` entries: the values and 1-byte codes, 2-byte codes or 4-byte columns
static size_t slice_lds(int cap, size_t V, int ienc) {
    return ienc == 8 ? (((size_t)cap * (V + 1) + 15) & ~(size_t)15) : ienc == 16 ? (((size_t)cap * (V + 2) + 15) & ~(size_t)15) : (size_t)cap * (V + 4);
}

SpmvForm choose_spmv_form(const SpmvPlan &plan, const Tuning &t, const SpmvCall &c) {
    const size_t V = (size_t)c.value_bytes;
    const int n = c.n, nrhs = c.nrhs;
    const bool vec = c.vec, fuse = c.fuse, rb_list = c.rb_list;
    SpmvForm f;
    f.fused = fuse; f.parts = plan.row_blocks;
    // CGAMD_SPLIT_LONG_ROWS: the regular blocks by their own kernel on the block list, then the heavy blocks' two launches (long_rows.hip).
    // The form is the split's, with the body's width, index encoding and grid
    if (plan.lr.on && vec && nrhs == 1 && !rb_list) {
        f.family = 9; f.vec = 1; f.nt = spmv_nt_now(t, plan);
        f.body = plan.lr.n_regular > 0;
        if (f.body) {
            SpmvCall bc = c;
            bc.rb_list = true; bc.rb_count = plan.lr.n_regular;
            const SpmvForm b = choose_spmv_form(long_rows_body(plan), t, bc);
            f.width = b.width; f.ienc = b.ienc; f.grid = b.grid;
        }
        return f;
    }
    if (vec && ((nrhs == 1 && plan.kind == 5) || (nrhs > 1 && plan.kind == 6 && plan.wide))) {
        f.cap = (plan.max_span + 3) & ~3;
        f.cycle = spmv_cycle_now(t);
        if (rb_list && c.rb_count <= 0) return f;      // nothing to launch
        f.vec = 1; f.nt = spmv_nt_now(t, plan);
        // one-byte column codes instead of aCols (build_index_codes; the codes belong to THIS cols array)
        const bool coded_any = nrhs == 1 && plan.codes && c.codes_for && t.index_codes != 0;
        const bool coded = coded_any && !plan.codes16;
        // ... and one-byte value codes on top (matrices of at most 256 distinct entries; complex128 has none)
        // (its staging covers slices of at most 8 x 256 entries: rows of 8 entries on average)
        const bool vcoded = coded && !rb_list && plan.vcodes && c.vcodes_for && t.value_codes != 0 && f.cap <= 8 * kBlock && (unsigned long long)n * V < (1ULL << 30);
        // up to 8 gathers in flight per lane for 4/8-byte values; 4 for complex128 (8 would cost 3 waves/SIMD of occupancy).  A row is
        // walked in batches of `unroll` slots (slots past the row's end re-read its last entry and are dropped): when no row of the
        // matrix is longer than 5 or 7 entries (5-point, 7-point and P1-FE stencils) the batch is exactly that long -- one batch per
        // row and no idle slot (N = 10M 7-point fp64: SpMV 134.7 -> 131.2 us, CG 4 215 -> 4 292 it/s; same sums, same bits)
        const int unroll = t.spmv_unroll ? t.spmv_unroll : (V > 8 ? 4 : batch_fit(plan.max_row));
        const int batch = unroll == 4 || unroll == 5 || unroll == 7 ? unroll : 8;      // the instances there are
        if (V <= 8 && vcoded) {
            const int supers = (plan.row_blocks + kVcBlocks - 1) / kVcBlocks;
            f.cycle = std::max(1, f.cycle / kVcBlocks);
            const int gvc = rowblock_grid(supers, f.cycle);
            f.ienc = 8;
            // rows that fit one batch (max_row <= unroll): the form with the gathers pipelined across the row blocks
            const bool pipe = plan.max_row > 0 && plan.max_row <= unroll && t.dev_vc_pipe != 0;
            // ... and where at most 256 (offset, value) pairs occur: one joint code byte per non-zero
            const bool joint = pipe && plan.jcodes && t.dev_joint_codes != 0;
            // ... and where the rows follow at most 256 patterns: one byte per ROW (build_row_codes), no row pointers and no code staging
            const bool rowform = joint && plan.rcodes && c.rcodes_for && t.dev_row_codes != 0;
            if (rowform) {
                // ... whose super blocks the handle's plane-matched table deals to the XCDs where it has one (solver.cpp
                // setup_xcd_schedule); the grid is the table's
                f.table = plan.sched != nullptr;
                f.grid = f.table ? plan.sched_grid : gvc;
                f.width = unroll; f.venc = 3;
                // ... and two rows per lane on one byte per PAIR of rows (build_row_pairs) where the vectors allow 16-byte accesses
                // (a caller's Solver.spmv vectors may not: the row form takes those)
                if (plan.pcodes && plan.pdict && plan.n_pair_patterns > 0 && row_pairs_wanted(t.dev_row_pairs, V) && n >= 2 && c.x16 && c.y16 &&
                    (!fuse || c.d16)) {
                    f.family = 8;
                    f.depth = std::min(2, row_pipe_depth(t.dev_row_pipe, V));       // dev.row_pipe's depth, 4 meaning 2 here
                    f.pair_slots = plan.pair_slots <= 7 ? 7 : 8;
                    f.lds = pair_dict_stage_bytes(plan.n_pair_patterns, V);
                    return f;
                }
                f.family = 7;
                f.depth = row_pipe_depth(t.dev_row_pipe, V);      // row blocks whose gathers are in flight per wave (0 = the default rule)
                f.lds = (size_t)plan.n_patterns * (8 * V + 8 * sizeof(int) + sizeof(int));
                return f;
            }
            f.family = pipe ? 3 : 2; f.width = batch; f.venc = joint ? 2 : 1; f.grid = gvc;
            f.lds = (((size_t)f.cap * 4 * kVcRows + 15) & ~(size_t)15) + 16;      // two buffers x kVcRows blocks x two code streams (+ the unclamped reads' slack)
            return f;
        }
        f.family = 1; f.width = batch; f.ienc = coded_any ? (plan.codes16 ? 16 : 8) : 0;
        f.grid = rb_list ? c.rb_count : rowblock_grid(plan.row_blocks, f.cycle);
        f.grid_y = nrhs; f.wide = nrhs > 1;
        f.lds = slice_lds(f.cap, V, f.ienc);
        return f;
    }
    if (vec && nrhs == 1 && plan.kind == 7) {
        if (rb_list && c.rb_count <= 0) return f;
        const int lpr = plan.lpr == 2 || plan.lpr == 4 || plan.lpr == 8 || plan.lpr == 16 ? plan.lpr : 32;
        const int span = plan.chunk_span[lpr == 2 ? 0 : lpr == 4 ? 1 : lpr == 8 ? 2 : lpr == 16 ? 3 : 4];
        f.family = 4; f.vec = 1; f.width = lpr; f.nt = spmv_nt_now(t, plan);
        f.cap = (span + 3) & ~3;
        f.cycle = spmv_cycle_now(t);
        f.ienc = plan.codes && c.codes_for && t.index_codes != 0 ? (plan.codes16 ? 16 : 8) : 0;
        f.lds = slice_lds(f.cap, V, f.ienc);
        f.grid = rb_list ? c.rb_count : rowblock_grid(plan.row_blocks, f.cycle);
        return f;
    }
    if (vec && nrhs > 1 && plan.kind == 6) {
        f.family = 5; f.vec = 1; f.nt = spmv_nt_now(t, plan);
        f.cap = (plan.max_span + 3) & ~3;
        f.cycle = spmv_cycle_now(t);
        f.lds = (size_t)f.cap * (V + 4) + (size_t)c.acc_bytes * nrhs * (kBlock / 64);
        f.grid = rowblock_grid(plan.row_blocks, f.cycle);
        const int rbmax = V <= 8 ? 8 : 4;
        // One launch covers all right-hand sides (groups of RB inside the kernel).  Splitting into one launch per
        // group (cgamd_tune "spmm_rb") re-reads the matrix per group and shrinks the x window per XCD; measured
        // slower at nRHS = 32 (253 vs 220 us) and at nRHS = 9 -- kept as an experiment knob only.
        f.chunk = (t.spmm_rb > 0 && t.spmm_rb < nrhs) ? t.spmm_rb : nrhs;
        // group width: the right-hand sides are cut into ceil(n / RBMAX) groups of (nearly) equal width, so that the last
        // group is not mostly padding -- the reference's own shape, 9 sub-domains, runs as 5 + 4 instead of 8 + 1
        const int ngroups = (f.chunk + rbmax - 1) / rbmax;
        int rbw = t.spmm_group > 0 ? t.spmm_group : (f.chunk + ngroups - 1) / ngroups;
        if (rbw > rbmax) rbw = rbmax;
        // (the instances there are: 8, 6, 5, 4, 3, 2; complex128: 4, 3, 2)
        f.width = rbmax == 8 && rbw > 6 ? 8 : rbmax == 8 && rbw >= 5 ? rbw : rbw >= 4 ? 4 : rbw == 3 ? 3 : 2;
        return f;
    }
    f.family = 0; f.vec = vec; f.grid = plan.grid; f.parts = plan.grid;      // (the stream kernel has no NT parameter)
    f.lds = (fuse && nrhs > 1) ? (size_t)c.acc_bytes * nrhs * (kBlock / 64) : 0;
    return f;
}

// Every input of the decision, once, in the order of the flat array: F(an int or bool), P(a pointer: only whether there is one).
// The names of cgamd_solver_spmv_form's inputs are these expressions as written (the array's declared size checks their number)
#define CG_FORM_INPUTS(F, P)                                                                                                          \
    F(c.value_bytes) F(c.acc_bytes) F(c.n) F(c.nrhs) F(c.vec) F(c.codes_for) F(c.vcodes_for) F(c.rcodes_for) F(c.fuse) F(c.rb_list)   \
    F(c.rb_count) F(c.x16) F(c.y16) F(c.d16)                                                                                          \
    F(plan.grid) F(plan.row_blocks) F(plan.max_span) F(plan.kind) F(plan.chunk_span[0]) F(plan.chunk_span[1]) F(plan.chunk_span[2])   \
    F(plan.chunk_span[3]) F(plan.chunk_span[4]) F(plan.wide) F(plan.max_row) F(plan.lpr) F(plan.nt) P(plan.codes) F(plan.codes16)     \
    P(plan.vcodes) P(plan.jcodes) P(plan.rcodes) F(plan.n_patterns) P(plan.pcodes) P(plan.pdict) F(plan.n_pair_patterns)              \
    F(plan.pair_slots) P(plan.sched) F(plan.sched_grid)                                                                               \
    F(plan.lr.on) F(plan.lr.n_regular) F(plan.lr.body_kind) F(plan.lr.body_lpr) F(plan.lr.body_max_span) F(plan.lr.body_max_row)      \
    F(plan.lr.body_chunk_span[0]) F(plan.lr.body_chunk_span[1]) F(plan.lr.body_chunk_span[2]) F(plan.lr.body_chunk_span[3])           \
    F(plan.lr.body_chunk_span[4])                                                                                                     \
    F(t.index_codes) F(t.value_codes) F(t.dev_joint_codes) F(t.dev_row_codes) F(t.dev_row_pipe) F(t.dev_row_pairs) F(t.dev_vc_pipe)   \
    F(t.spmv_nt) F(t.spmv_cycle) F(t.spmv_unroll) F(t.spmm_rb) F(t.spmm_group)
#define CG_NAME(x) #x,
const char *const kSpmvFormInputNames[] = {CG_FORM_INPUTS(CG_NAME, CG_NAME)};
#define CG_PACK(x) *out++ = (int)(x);
#define CG_PACK_PTR(x) *out++ = (x) != nullptr;
void spmv_form_pack(const SpmvPlan &plan, const Tuning &t, const SpmvCall &c, int *out) { CG_FORM_INPUTS(CG_PACK, CG_PACK_PTR) }
// (a restored pointer points to `some`: the decision only asks whether there is one)
#define CG_UNPACK(x) x = static_cast<std::remove_reference_t<decltype((x))>>(*in++);
#define CG_UNPACK_PTR(x) x = *in++ ? reinterpret_cast<decltype(x)>(&some) : nullptr;
void spmv_form_unpack(const int *in, SpmvPlan *plan_out, Tuning *t_out, SpmvCall *c_out) {
    static const unsigned char some = 0;
    SpmvPlan &plan = *plan_out;
    Tuning &t = *t_out;
    SpmvCall &c = *c_out;
    CG_FORM_INPUTS(CG_UNPACK, CG_UNPACK_PTR)
}

} // namespace cgamd
