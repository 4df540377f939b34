// rank_math.h — the small integer arithmetic of the rank planes (include/chanvese_hip.h, "Rank planes") that the kernels
// (rank_kernels.hip) and the host (window_run.hip; debug_exports.hip, which tests/test_rank_api.py and tests/test_rank_restatement.py hold
// against Python integers) share: which chain of erosions and dilations a code needs, the rows of a column band at a radius, the rank of
// the lower median, and the walk over sixteen packed byte counters that finds the bin of a rank.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVH_RANK_FN __host__ __device__ inline
#else
#define CVH_RANK_FN inline
#endif

// The chain a code is built from: 0 starts with an erosion (MIN, OPEN, TOPHAT), 1 with a dilation (MAX, CLOSE, BOTHAT), -1 neither
// (COPY, MEDIAN).  The codes are the header's: 1 MIN, 2 MAX, 4 OPEN, 5 CLOSE, 6 TOPHAT, 7 BOTHAT.
CVH_RANK_FN int cvh_rank_chain(int code) { return code == 1 || code == 4 || code == 6 ? 0 : code == 2 || code == 5 || code == 7 ? 1 : -1; }
// whether the chain runs twice (erosion then dilation, or the reverse): OPEN, CLOSE and the two hats
CVH_RANK_FN int cvh_rank_twice(int code) { return code >= 4 && code <= 7; }

// rows of a band of the column passes at radius R: the least multiple of the van Herk block 2 R + 1 that is not below `band`, so that
// every band starts on a block seam and its start-up does not grow with R
CVH_RANK_FN int cvh_rank_band_rows(int R, int band) { const int K = 2 * R + 1; return K * ((band + K - 1) / K); }

// the index of the lower median among n sorted samples
CVH_RANK_FN uint32_t cvh_rank_median_index(uint32_t n) { return (n - 1) / 2; }

// Sixteen byte counters packed in w[0 .. 3], lowest byte first: the index of the first counter at which the running count, begun at
// *before, exceeds t (16: none does), and in *before the count in front of that counter
CVH_RANK_FN int cvh_rank_walk(const uint32_t w[4], uint32_t *before, uint32_t t)
{
  uint32_t cum = *before;
  int at = 16;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 16; ++i) {
    const uint32_t cnt = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
    const bool here = at == 16 && cum + cnt > t;
    if (here) at = i;
    if (at == 16) cum += cnt;
  }
  *before = cum;
  return at;
}
