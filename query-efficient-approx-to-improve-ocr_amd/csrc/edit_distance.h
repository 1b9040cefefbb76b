// Unit-cost edit distance, one problem per lane of a 64-lane workgroup: misc.hip's edit_distance_kernel (CER numerator) and
// history.hip's history_lev_kernel (label-history weights) run this one recursion and differ only in where a character comes from.
#pragma once
#include "common.h"

constexpr int ED_MAX = QEA_HISTORY_MAX_LEN;                // longest inner word: the LDS row holds (ED_MAX + 1) * 64 ints
constexpr int ED_LANES = 64;

// D[la][lb] of the lane's two words; outer(i) / inner(j) return character i / j.  The lane's DP row sits in LDS column-major
// (row[j * 64 + lane]: conflict-free) and needs lb <= ED_MAX; la is free.
template <class Outer, class Inner>
__device__ __forceinline__ int edit_distance_lane(int* row, int lane, int la, int lb, Outer outer, Inner inner) {
  for (int j = 0; j <= lb; ++j) row[j * ED_LANES + lane] = j;
  for (int i = 1; i <= la; ++i) {
    const int ca = outer(i - 1);
    int diag = row[lane];  // D[i-1][0]
    row[lane] = i;
    int left = i;
    for (int j = 1; j <= lb; ++j) {
      const int up = row[j * ED_LANES + lane];
      const int v = min(min(up + 1, left + 1), diag + (inner(j - 1) != ca));
      row[j * ED_LANES + lane] = v;
      diag = up;
      left = v;
    }
  }
  return row[lb * ED_LANES + lane];
}
