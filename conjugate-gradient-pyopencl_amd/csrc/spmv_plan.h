// What the SpMV launchers and the form decision (spmv_form.h) share: the plan of a matrix, the run-time tuning, and the constants and
// one-line rules both read.  No HIP in here.
#pragma once
#include <cstddef>

namespace cgamd {

// Launch geometry shared by every SpMV form.
constexpr int kBlock = 256;          // threads per work-group (4 waves)
constexpr int kSuperRows = 4 * kBlock;   // rows of a SUPER block: the kVcBlocks row blocks one work-group of the coded SpMV forms takes (spmv.hip)

// CGAMD_SPLIT_LONG_ROWS (long_rows.hip): the 256-row blocks no block form can hold ("heavy") run a segmented kernel pair, every other
// block the row-block or chunked kernel through a block list.  Device lists, built once from the row pointers and owned by the handle
struct LongRows {
    int on = 0;                     // the handle's single-RHS SpMV takes the split form
    int n_heavy = 0, n_seg = 0, n_regular = 0;
    int seg_len = 0;                // entries per segment (a multiple of 4)
    int body_kind = 0, body_lpr = 1;                // the regular blocks' kernel (5 or 7) and its lanes per row, from THEIR spans:
    int body_max_span = 0, body_max_row = 0, body_chunk_span[5] = {0, 0, 0, 0, 0};
    int *regular = nullptr;         // [n_regular] regular row blocks in the order rowblock_of deals them
    int *heavy = nullptr;           // [n_heavy] heavy row blocks, ascending
    int *seg0 = nullptr;            // [n_heavy + 1] first segment of every heavy block
    int *segtab = nullptr;          // [n_seg][2]: heavy block (index into heavy[]), first entry (4-aligned)
    void *scratch = nullptr;        // [n_seg][2] values: the pieces of the (at most two) rows that cross a segment's edges
    size_t scratch_bytes = 0;
};
struct SpmvPlan {
    LongRows lr;
    int grid = 0;        // work-groups launched (multiple of 8 when >= 8)
    int row_blocks = 0;  // ceil(n / kBlock)
    int max_span = 0;    // largest 4-aligned nnz span of a kBlock-row slice (0 = unknown -> generic kernel)
    int kind = 0;        // kernel chosen by finalize_spmv_plan (0 generic, 5 row-block, 6 its SpMM form, 7 chunked row-block)
    int chunk_span[5] = {0, 0, 0, 0, 0};   // largest 4-aligned span of a 128 / 64 / 32 / 16 / 8-row slice
    bool wide = false;   // kind 6 only: small system, one work-group per (row block, RHS) runs the single-RHS kernel
    int max_row = 0;     // longest row (0 = unknown): the row-block kernel's batch length follows it
    int max_quad = 0;    // most non-zeros in 4 consecutive rows starting at a multiple of 4 (row-major SpMM: K-steps per quad)
    int lpr = 1;         // kind 7: lanes per row (2, 4, 8, 16, 32) = chunks per 256-row block
    int n_partials = 0;  // fused-dot partials per RHS written by that kernel
    int fold_max = 0;    // most d.q partials the folded alpha sums (0 = default; handles the chip-wide resident loop takes over: 4096)
    int nt = 1;          // matrix stream loaded non-temporally (finalize_spmv_plan: off when the matrix fits the Infinity Cache)
    int vec_nt = 3;      // axpy2_dot streaming hints (see Tuning::vec_nt), resolved by finalize_spmv_plan
    // one-byte column codes of the single-RHS row-block kernel (build_index_codes; owned by the caller, not by the plan)
    const unsigned char *codes = nullptr;   // [nnz + pad]: aCols[j] = row(j) + dict[codes[j]]
    const int *dict = nullptr;              // [256] distinct (column - row) offsets of the matrix
    const int *codes_for = nullptr;         // the aCols array the codes were made from
    bool codes16 = false;                   // the codes are 16-bit columns relative to the row block's first column (build_index_codes16)
    // one-byte VALUE codes (build_value_codes; with the one-byte column codes only): aValues[j] == vdict[vcodes[j]]
    const unsigned char *vcodes = nullptr;  // [nnz + pad]
    const void *vdict = nullptr;            // [256] values
    const void *vcodes_for = nullptr;       // the aValues array the codes were made from
    // one-byte JOINT codes (build_joint_codes): (aCols[j] - row, aValues[j]) == (jdict_off[jcodes[j]], jdict_val[jcodes[j]])
    const unsigned char *jcodes = nullptr;  // [nnz + pad]
    const int *jdict_off = nullptr;         // [256] offsets
    const void *jdict_val = nullptr;        // [256] values
    // one-byte ROW-PATTERN codes (build_row_codes): row i multiplies the rdict_len[c] pairs (rdict_off[c][j], rdict_val[c][j]), c = rcodes[i]
    const unsigned char *rcodes = nullptr;  // [n + pad]
    const int *rdict_len = nullptr;         // [256] entries of the pattern
    const int *rdict_off = nullptr;         // [256][8] column offsets in BYTES (times the size of a value)
    const void *rdict_val = nullptr;        // [256][8] values
    int n_patterns = 0;                     // patterns that occur (the kernel stages only these)
    const int *rcodes_for = nullptr;        // the aPointers array the codes were made from (with codes_for / vcodes_for: the matrix)
    // one-byte ROW-PAIR codes on top of the row codes (build_row_pairs): rows 2p and 2p + 1 follow pair pattern pcodes[p] of pdict
    const unsigned char *pcodes = nullptr;  // [ceil(n / 2) + pad]
    const void *pdict = nullptr;            // pair_dict_* layout, n_pair_patterns entries
    int n_pair_patterns = 0;
    int pair_slots = 0;                     // the longest union of slots among the pair patterns (the kernel walks 7 or 8)
    // PLANE-MATCHED schedule of the row- and pair-coded kernels (build_xcd_schedule, xcd_schedule.h): work-group b takes super block
    // sched[b] (-1: none); null = the block-cyclic schedule of rowblock_of
    const int *sched = nullptr;             // [sched_grid]
    int sched_grid = 0;
};

// layout of the row-pair dictionary (build_row_pairs, cgamd_internal.h): what the pair kernel stages is pair_dict_stage_bytes
constexpr size_t pair_dict_val1_at(int np, size_t value_size) { return (size_t)np * 8 * value_size; }
constexpr size_t pair_dict_off_at(int np, size_t value_size) { return 2 * (size_t)np * 8 * value_size; }
constexpr size_t pair_dict_mask_at(int np, size_t value_size) { return pair_dict_off_at(np, value_size) + (size_t)np * 8 * sizeof(int); }
constexpr size_t pair_dict_stage_bytes(int np, size_t value_size) { return pair_dict_mask_at(np, value_size) + (size_t)np * sizeof(int); }
constexpr size_t pair_dict_src_at(int np, size_t value_size) { return pair_dict_stage_bytes(np, value_size); }
constexpr size_t pair_dict_alloc_bytes(int np, size_t value_size) { return pair_dict_src_at(np, value_size) + (size_t)np * 16 * sizeof(unsigned short); }

// run-time tuning (cgamd_tune); defaults are the shipped configuration.  PUBLIC keys (include/cgamd.h): the 15
// of the first block.  The second block are development hooks (key prefix "dev."): what the tests need to force a loop family or a
// failure, and rehearsal switches; experiments that were decided have no knob any more.
struct Tuning {
    // ---- public
    int index_codes = 1;    // single-RHS row-block SpMV on one-byte column codes (0 = always aCols)
    int index_codes16 = 1;  // ... and, where the matrix has more than 256 offsets, on 16-bit block-relative columns (0 = aCols then)
    int index_codes_min_mb = 32;    // ... for matrices above this size (smaller systems run the resident / two-launch loops, which read aCols)
    int resident = 1;       // systems of at most 32768 rows whose matrix slices fit LDS: all iterations of an iterate() call in ONE launch
                            // (resident.hip); 0 = never, 2 = always in the cross-XCD form (up to 65536 rows; for the any-placement tests)
    int resident_min = 8;   // ... for iterate() calls of at least this many iterations
    int resident_wide = 1;  // systems the one-XCD loop cannot hold (rows of <= 10 entries, up to ~1M rows): chip-wide resident groups; 0 = launched
    int resident_wide_min = 16; // ... for iterate() calls of at least this many iterations (also the slab loop's threshold, slab.hip)
    int resident_claim_ms = 200;   // resident loops: how long a call waits for the GPU's resident-launch lock, and work-groups for their group to
                               // fill (CUs held by other kernels), before the launch gives up untouched and the handle takes the launched loops
    int two_launch = 1;     // small systems: beta / d = beta d + r inside the next SpMV launch, two launches per iteration (0 = three / four)
    int spmm_rowmajor = 1;  // 1: solvers keep the block row-major where that loop is the faster one (f64 x 32); 2: for every supported type
                            // (f32 16/32/64, f64 16/32, complex64 16/32); 0: never
    int pad_rows = 1;       // sizes that are not whole 16-byte packs are carried with 1-3 empty rows appended (0 = as passed)
    int spmv_nt = -1;       // non-temporal matrix loads: 1 on, 0 off, -1 auto = on unless the matrix fits the 256 MB Infinity Cache
    int vec_nt = -1;        // -1 auto (by working-set size); bit0 = x loaded/stored non-temporally, bit1 = q loaded non-temporally
    int spmv_cycle = 64;    // row-block schedule: block-cyclic over the XCDs, cycle length in row blocks (1 = contiguous eighths)
    int vec_grid = 0;       // vector kernels: work-groups, 0 = auto
    // ---- development hooks ("dev." keys): tests, rehearsals, profiling
    int dev_no_fold_alpha = 0;      // 1: small systems keep the separate cg_alpha launch (the four-launch family at sizes that would fold it)
    int dev_x_lag = -1;             // captured runs of the three / four-launch loop bring x up to date once per this many iterations: 2, 4 or 8;
                                    // 0 / 1 = every iteration; -1 = the default rule (solver.cpp x_lag_wanted)
    int dev_x_lag_dnt = 1;          // ... the last step of a group loads the direction buffers, read for the last time, non-temporally where x streams
                                    // too (0 = plain loads: A/B, profiles/x_lag/ab.log: lag 4 5970 -> 6059 it/s at 10M rows fp64, no difference at 100M)
    int value_codes = 1;            // one-byte value codes on top of the one-byte column codes where the matrix has at most 256 distinct entries (0 = off: A/B, tests)
    int dev_joint_codes = 1;        // value-coded SpMV: one byte per non-zero naming the (offset, value) pair where at most 256 pairs occur (0 = two bytes: A/B)
    int dev_row_codes = 1;          // joint-coded SpMV: one byte per ROW naming its pattern where at most 256 row patterns occur (0 = joint codes: A/B)
    int dev_row_codes_min_mb = 32;  // ... for matrices above this size (its own threshold: index_codes_min_mb = 0 alone keeps the joint form)
    int dev_row_pipe = 0;           // row-coded SpMV: row blocks whose gathers are in flight per wave, 1, 2 or 4 (0 = the default rule, row_pipe_depth)
    int dev_row_pairs = -1;         // row-coded SpMV: two rows per lane on one byte per PAIR of rows, one 16-byte gather per slot (1 / 0; -1 = the default rule, row_pairs_wanted)
    int dev_row_pairs_min_mb = 256; // ... for matrices above this size (a threshold of its own, like dev_row_codes_min_mb).  256 MB: every system the
                                    // form was measured on lies above it (300 MB, 840 MB, 8.4 GB: profiles/row_pairs/), and the handles of 85 to 151 MB
                                    // whose CG steps are tested bit for bit (tests/test_gpu_cg_steps.py) keep recording the row form they assert
    int dev_spmv_plane = -1;        // row- and pair-coded SpMV: super blocks dealt to the XCDs by their place inside the handle's largest stride, from a
                                    // table per handle (1: every such handle; 0: the block-cyclic schedule; -1 = the default rule, spmv_plane_wanted)
    int dev_vc_pipe = 1;            // value-coded SpMV: gathers pipelined across the row blocks of a work-group (0 = one block at a time: A/B)
    int dev_generic_spmv = 0;       // 1: the generic chunked CSR stream for every matrix (the row-block kernels' fallback, tested against them)
    int dev_long_row_bytes = 0;     // CGAMD_SPLIT_LONG_ROWS: an 8-row slice of more than this many bytes makes its row block heavy (0 = kMaxChunkBytes;
                                    // larger values count as that: the threshold can only be lowered, so that tests reach the form at small shapes)
    int dev_long_row_segment = 0;   // ... entries per segment, a multiple of 4 (0 = kLongRowSegment)
    int resident_lock = 1;          // 0: no per-GPU serialisation of resident launches (ranks of ONE job sharing a GPU in a rehearsal)
    int slab_trim = -1;             // slab loop: 1024-row granules a member that pushes to a peer owns fewer than the others (-1 = 2, 0 = equal members)
    int slab_cus = 0;               // slab loop: CUs (= members at most) a handle may use; 0 = all (ranks that share a GPU must fit side by side)
    int resident_test_short_grid = 0; // launch one work-group too few, so that no group can fill (the untouched-fallback tests)
    int resident_wide_rpt = 0;      // rows per thread of the chip-wide loop: 0 = the smallest that fits (4, then 8), or 4 / 8
    int resident_window = 1;        // one-XCD resident loop: stage the column range of a member's rows in LDS (0 = per-non-zero gathers)
    int vec_ppt = 0;                // vector kernels: 16-byte packs per thread the grid is sized for (0 = by size: 1, 2 or 4)
    int spmv_unroll = 0;            // row walk: gathers in flight per lane (0 = fitted to the longest row)
    int spmv_grid = 0;              // generic kernel: work-groups, 0 = auto
    int spmv_slice_kb = 0;          // largest 256-row LDS slice the one-lane-per-row kernel accepts, in KB (0 = kMaxSliceBytes)
    int spmv_chunk_kb = 0;          // chunked row-block kernel: preferred LDS chunk in KB (0 = kChunkBytes)
    int spmv_chunked = 1;           // rows too dense for the row-block kernel: chunked row-block kernel (0 = generic kernel)
    int spmm_ynt = -1;              // row-major SpMM y stores: 0 plain, 1 non-temporal, 2 write-through sc1 (-1 = default: 2)
    int spmm_group = 0;             // SpMM: right-hand sides per register group (0 = equal-width groups of at most 8, 4 for complex128)
    int spmm_rb = 0;                // SpMM: right-hand sides per launch (0 = all in one launch)
    int spmm_wgs = 0;               // row-major SpMM sweep: work-groups per XCD (0 = 64)
    int spmm_lead = 0;              // row-major SpMM sweep: steps a wave may gather ahead of its XCD's slowest (0 = default, -1 = unpaced)
    int spmm_wide_max = -1;         // multi-RHS, RHS-major: largest row_blocks x nRHS for the one-work-group-per-RHS form (-1 = 4096, 0 = never)
    int dev_line_host_route = 0;    // cgamd_solver_set_preconditioner_line: 1 = extract on the device, factor and plan by the host route (source 3)
};
// the depth the row-coded SpMV launches with under dev.row_pipe = `knob`: 1, 2 and 4 as given, anything else the default rule --
// by the size of a value, as measured (profiles/row_pipe/): 4-byte values all four blocks; 8-byte values one block at a
// time (two measured 0.1 to 1.1 % faster in one process, but the plain benchmark did not separate it from the parent build by the
// margin asked for, so the depth of 8-byte values stays at 1)
inline int row_pipe_depth(int knob, size_t value_bytes) { return knob == 1 || knob == 2 || knob == 4 ? knob : value_bytes <= 4 ? 4 : 1; }
// whether a handle builds and launches the row-pair form under dev.row_pairs = `knob`: 1 and 0 as given, anything else the default
// rule -- by the size of a value, as measured (profiles/row_pairs/)
inline bool row_pairs_wanted(int knob, size_t value_bytes) { return knob == 1 ? true : knob == 0 ? false : value_bytes >= 8; }

// ---- the three one-line rules every SpMV launcher shares ----
// matrix stream loaded non-temporally NOW: the knob where it is set, else what finalize_spmv_plan decided from the matrix's size
inline bool spmv_nt_now(const Tuning &t, const SpmvPlan &plan) { return t.spmv_nt >= 0 ? t.spmv_nt != 0 : plan.nt != 0; }
// cycle of the block-cyclic row-block schedule, in row blocks
inline int spmv_cycle_now(const Tuning &t) { return t.spmv_cycle > 0 ? t.spmv_cycle : 1; }
// batch length of the row walk fitted to the longest row: one batch per row of a 5- / 7-point stencil and no idle slot (0 = unknown: 8)
inline int batch_fit(int max_row) { return max_row <= 0 ? 8 : max_row <= 4 ? 4 : max_row == 5 ? 5 : max_row <= 7 ? 7 : 8; }

// work-groups of the row-block schedule (spmv_device.h rowblock_of): the padded grid that deals `row_blocks` blocks to 8 XCDs
inline int rowblock_grid(int row_blocks, int cycle) {
    if (cycle > 1) return 8 * ((cycle + 7) / 8) * ((row_blocks + cycle - 1) / cycle);
    int per_xcd = 0;
    for (int x = 0; x < 8; ++x) {
        const int m = (int)((long long)(x + 1) * row_blocks / 8) - (int)((long long)x * row_blocks / 8);
        per_xcd = m > per_xcd ? m : per_xcd;
    }
    return per_xcd * 8;
}
constexpr int kVcBlocks = 4;      // row blocks per work-group of the value-coded, row-coded and pair-coded kernels
static_assert(kVcBlocks * kBlock == kSuperRows, "the plane-matched schedule (solver.cpp) counts super blocks of kSuperRows rows");
constexpr int kVcRows = 1;        // of which a thread walks this many at a time (one row of each): 2 were measured slower (108 VGPRs)

} // namespace cgamd
