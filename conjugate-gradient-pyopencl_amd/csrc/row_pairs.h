// Host side of the ROW-PAIR patterns (row_pairs.cpp): the union of the slots of two consecutive rows.  No HIP in here: the merge is
// compiled into the libraries and, for its CPU test, into a stand-alone program.
#pragma once

namespace cgamd {

constexpr int kPairSlots = 8;       // union slots a pair pattern holds at most

// The slots of a pair of rows (2p, 2p + 1): a shortest common supersequence of the two rows' stored slot sequences keyed by the
// offset (column - row), so that each row's stored order survives as a subsequence and two slots merge exactly when their offsets
// are equal.  src0[u] / src1[u]: the stored slot of row 2p / 2p + 1 that union slot u serves, or -1 where that row does not use it.
struct PairPattern {
    int n;
    int off[kPairSlots], src0[kPairSlots], src1[kPairSlots];
};
// false: the shortest common supersequence is longer than kPairSlots (out->n then holds its length).  len0, len1 in [0, 8].
bool merge_pair_slots(int len0, const int *off0, int len1, const int *off1, PairPattern *out);

}  // namespace cgamd
