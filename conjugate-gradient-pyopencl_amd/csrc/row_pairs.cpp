// ROW-PAIR patterns, host side: merge the slot sequences of two consecutive rows into one sequence of at most kPairSlots union slots
// (row_pairs.h).  Plain C++; index_codes.hip builds the pair dictionary with it.
#include "row_pairs.h"

namespace cgamd {

// lcs[i][j] = longest common subsequence of off0[i..] and off1[j..]; the walk from the front emits a merged slot wherever the two
// heads are equal (always part of some longest common subsequence), else the head whose removal keeps the longer common
// subsequence -- row 2p's on a tie.  The result has len0 + len1 - lcs[0][0] slots, which is the shortest possible.
bool merge_pair_slots(int len0, const int *off0, int len1, const int *off1, PairPattern *out) {
    constexpr int M = 8;
    out->n = 0;
    for (int u = 0; u < kPairSlots; ++u) { out->off[u] = 0; out->src0[u] = -1; out->src1[u] = -1; }
    if (len0 < 0 || len1 < 0 || len0 > M || len1 > M) { out->n = kPairSlots + 1; return false; }
    int lcs[M + 1][M + 1];
    for (int i = len0; i >= 0; --i)
        for (int j = len1; j >= 0; --j) {
            if (i == len0 || j == len1) lcs[i][j] = 0;
            else if (off0[i] == off1[j]) lcs[i][j] = lcs[i + 1][j + 1] + 1;
            else lcs[i][j] = lcs[i + 1][j] >= lcs[i][j + 1] ? lcs[i + 1][j] : lcs[i][j + 1];
        }
    const int total = len0 + len1 - lcs[0][0];
    if (total > kPairSlots) { out->n = total; return false; }
    int i = 0, j = 0, u = 0;
    while (i < len0 || j < len1) {
        if (i < len0 && j < len1 && off0[i] == off1[j]) { out->off[u] = off0[i]; out->src0[u] = i++; out->src1[u] = j++; }
        else if (j == len1 || (i < len0 && lcs[i + 1][j] >= lcs[i][j + 1])) { out->off[u] = off0[i]; out->src0[u] = i++; }
        else { out->off[u] = off1[j]; out->src1[u] = j++; }
        ++u;
    }
    out->n = u;
    return true;
}

}  // namespace cgamd
