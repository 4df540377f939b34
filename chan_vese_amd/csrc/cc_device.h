// cc_device.h — what the kernels that read a numbered forest or fill a cvh_component table share (components_kernels.hip,
// split_kernels.hip): the two marks of a parent word, the run of equal keys inside a wave, and a run's share of a table row.
#pragma once
#include <limits.h>

#include "cvh_internal.h"

namespace {

constexpr unsigned kCcNone = 0xffffffffu;       // parent word: not a pixel of the class
constexpr unsigned kCcNumbered = 0x80000000u;   // parent word of a root after cc_number_kernel: kCcNumbered | k, k = 1 .. K <= 2^30

// lanes i .. i + len - 1 of the wave hold the same key and lane i starts the run (len = 0: not a start); cut also starts a run
__device__ __forceinline__ unsigned cc_run_length(unsigned key, bool cut)
{
  const unsigned lane = threadIdx.x & 63u, prev = __shfl_up(key, 1, 64);
  const bool start = key != kCcNone && (lane == 0 || prev != key || cut);
  const unsigned long long ends = __ballot(start || key == kCcNone) & ~((2ull << lane) - 1ull);
  if (!start) return 0;
  return (ends ? (unsigned)__builtin_ctzll(ends) : 64u) - lane;
}

// a table row's neutral elements behind its `first`
__device__ __forceinline__ void cc_row_init(__attribute__((address_space(1))) cvh_component *row, unsigned first)
{
  row->first = first; row->area = 0;
  row->x0 = INT_MAX; row->y0 = INT_MAX; row->x1 = -1; row->y1 = -1;
}

// a horizontal run of len pixels from (r, c0) joins its row: one add, min and max only where they would move the value
__device__ __forceinline__ void cc_row_add_run(__attribute__((address_space(1))) cvh_component *row, unsigned len, int r, int c0)
{
  const int c1 = c0 + (int)len - 1;
  __hip_atomic_fetch_add(&row->area, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (c0 < __hip_atomic_load(&row->x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_min(&row->x0, c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (r < __hip_atomic_load(&row->y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_min(&row->y0, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (c1 > __hip_atomic_load(&row->x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_max(&row->x1, c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (r > __hip_atomic_load(&row->y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_max(&row->y1, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
