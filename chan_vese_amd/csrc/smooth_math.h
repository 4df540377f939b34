// smooth_math.h — the roundings of the weighted window (include/chanvese_hip.h, "Smoothing"): one set of inline functions for the kernels
// (smooth_kernels.hip) and for the host (debug_exports.hip: tests/test_smooth_restatement.py holds them against Python integers).  Taps
// are 15-bit fixed point and add up to 32768 over the whole window, so a tap-weighted sum of bytes is below 2^23 and one of row values
// (8.8 fixed point, at most 65280) is at most 65280 * 32768 < 2^31: both live in 32 unsigned bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVH_SMOOTH_FN __host__ __device__ inline
#else
#define CVH_SMOOTH_FN inline
#endif

// row pass: a = sum t[|i|] p <= 255 * 32768 -> v = (a + 64) >> 7 <= 65280
CVH_SMOOTH_FN uint32_t cvh_smooth_row(uint32_t a) { return (a + 64u) >> 7; }

// column pass: b = sum t[|j|] v <= 65280 * 32768 -> BLUR = (b + 2^22) >> 23 <= 255
CVH_SMOOTH_FN uint32_t cvh_smooth_blur(uint32_t b) { return (b + (1u << 22)) >> 23; }

// DETAIL = min(255, max(0, 128 + p - BLUR))
CVH_SMOOTH_FN uint32_t cvh_smooth_detail(uint32_t p, uint32_t blur)
{
  const int d = 128 + (int)p - (int)blur;
  return (uint32_t)(d < 0 ? 0 : d > 255 ? 255 : d);
}
