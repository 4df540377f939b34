// local_math.h — the per-pixel arithmetic of the local statistics (include/chanvese_hip.h, "Local statistics"), from the window's pixel
// count n, S = sum p and Q = sum p^2: one set of inline functions for the kernels (local_kernels.hip) and for the host
// (debug_exports.hip: tests/test_local_restatement.py holds them against Python integers, the square root over every argument).
// The header defines both statistics in unsigned 64-bit integers with floor division; these functions give exactly those values and
// replace the two long divisions by a floating-point estimate and an integer correction.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CVH_LOCAL_FN __host__ __device__ inline
#else
#define CVH_LOCAL_FN inline
#endif

// floor(sqrt(q)) for q <= 65025 (= 255^2): a float holds q exactly and its root is below 256, so the estimate is off by one at most;
// the two loops make it the floor whatever the estimate was
CVH_LOCAL_FN uint32_t cvh_local_isqrt(uint32_t q)
{
  uint32_t s = (uint32_t)sqrtf((float)q);
  while (s * s > q) --s;
  while ((s + 1) * (s + 1) <= q) ++s;
  return s;
}

// MEAN = (2 S + n) / (2 n): n <= 65025 and S <= 255 n, so 2 S + n < 2^25
CVH_LOCAL_FN uint32_t cvh_local_mean(uint32_t n, uint32_t S) { return (2u * S + n) / (2u * n); }

// DEV = isqrt(4 (n Q - S^2) / n^2).  V = 4 (n Q - S^2) < 2^51 and D = n^2 < 2^33 are exact doubles and V / D <= 65025, so the
// truncated double quotient misses floor(V / D) by one at most: the remainder says which way
CVH_LOCAL_FN uint32_t cvh_local_dev(uint32_t n, uint32_t S, uint32_t Q)
{
  const uint64_t V = 4ull * ((uint64_t)n * Q - (uint64_t)S * S), D = (uint64_t)n * n;
  uint64_t q = (uint64_t)((double)V / (double)D);
  while (q * D > V) --q;
  while ((q + 1) * D <= V) ++q;
  return cvh_local_isqrt((uint32_t)q);
}
