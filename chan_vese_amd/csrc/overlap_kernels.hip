// overlap_kernels.hip — the contingency table of cvh_overlaps* (include/chanvese_hip.h, "Component overlaps"; gfx950): for a NUMBERED forest
// (components_kernels.hip, behind cc_number_kernel) and a second label plane B of the caller's, the number of pixels of every pair
// (a, b) = (label of the forest, value of B) that occurs.  All integers, all sums: neither the grid, the schedule nor the hash below can
// change a count, and the ORDER of the rows is the host's sort (overlap_run.hip), not the order of the slots.
// A member's section is ceil(h w / CVH_MEASURE_TILE) workgroups; a workgroup makes CVH_MEASURE_TILE / 256 trips over its tile in flat
// raster order, so a wave holds 64 consecutive flat indices per trip (as the measure kernels).  Per trip a lane
//   reads its label (parent word, and the root's word where the pixel is no root) and its word of B: 8 bytes per pixel, once;
//   forms the 64-bit key ((a + 1) << 32) | (uint32_t)b -- a >= 0, so no key is 0, the EMPTY key, whose a-half decodes to -1;
//   the first lane of every run of equal keys inside the wave (a ballot: the sum of the run's ones is its length) adds the length to
//   the workgroup's table in LDS: kLds slots, open addressing, at most kLdsProbe probes; a run that finds no slot there goes to the
//   member's global table directly.
// After the last trip every occupied LDS slot goes to the global table once: a plane that is one pair costs one global atomic per
// WORKGROUP.  The global table is `slots` (a power of two) CvhOverlapSlot in the context's workspace: a key is claimed by a 64-bit
// compare-and-swap against the empty key, the count added by a 32-bit add, both plain vector atomics at agent scope.
// EVERY PROBE LOOP IS BOUNDED: kLdsProbe in LDS, `slots` in global memory.  The lane that claims the slot that makes the table more than
// half full, or that finds no slot, sets the member's overflow word; a lane that sees the word set inserts nothing more.  The host then
// runs the launch again on a larger table (overlap_run.hip).  Nothing here waits for or polls another workgroup.
#include "cvh_internal.h"

namespace {

#define CVH_GLOBAL __attribute__((address_space(1)))
typedef CVH_GLOBAL const unsigned *gwords;
typedef unsigned long long u64;

static_assert(CVH_BLOCK == 256 && CVH_MEASURE_TILE % CVH_BLOCK == 0, "a trip is four waves of 64 consecutive pixels");
static_assert(sizeof(CvhOverlapSlot) == 16 && sizeof(cvh_overlap) == 16, "a slot and a row are 16 bytes");
// components_kernels.hip's encoding of the parent words behind cc_number_kernel
constexpr unsigned kNone = 0xffffffffu;       // not a pixel of the class
constexpr unsigned kNumbered = 0x80000000u;   // a root: kNumbered | k, k = 1 .. K; every other pixel of the class holds its root's index
constexpr unsigned kLds = 512, kLdsProbe = 8; // slots of the workgroup's table (6 KiB), and how far a run looks for one
constexpr u64 kEmpty = 0;

__device__ __forceinline__ int overlap_member(const CvhIoMember *tab, int nmem)
{
  int lo = 0, hi = nmem - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ u64 upto(unsigned lane) { return (2ull << lane) - 1ull; }   // bits 0 .. lane (lane 63: all)

// the label of pixel p (0 outside the class)
__device__ __forceinline__ unsigned label_of(gwords parent, unsigned p)
{
  const unsigned v = parent[p];
  if (v == kNone) return 0;
  return ((v & kNumbered) ? v : parent[v]) & ~kNumbered;
}

__device__ __forceinline__ u64 mix(u64 x)
{
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
  return x ^ (x >> 33);
}

#define DEV_LOAD(P) __hip_atomic_load((P), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define DEV_ADD(P, V) __hip_atomic_fetch_add((P), (V), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// count pixels more of `key` in the member's global table.  ctl: [0] slots claimed so far, [1] the overflow word
__device__ __forceinline__ void global_add(CVH_GLOBAL CvhOverlapSlot *slots, u64 nslots, CVH_GLOBAL unsigned *ctl, u64 key, unsigned count)
{
  if (DEV_LOAD(ctl + 1)) return;   // (the launch is lost already: the host runs it again on a larger table)
  const u64 mask = nslots - 1;
  u64 i = mix(key) & mask;
  for (u64 probe = 0; probe < nslots; ++probe, i = (i + 1) & mask) {
    u64 cur = DEV_LOAD(&slots[i].key);
    if (cur == kEmpty) {
      if (__hip_atomic_compare_exchange_strong(&slots[i].key, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        if ((u64)DEV_ADD(ctl, 1u) + 1u > nslots / 2) __hip_atomic_store(ctl + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cur = key;
      }   // (else cur is the key that won the slot)
    }
    if (cur == key) { DEV_ADD(&slots[i].count, count); return; }
  }
  __hip_atomic_store(ctl + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every slot holds another key
}

// the same in the workgroup's table; false: no slot within kLdsProbe probes
__device__ __forceinline__ bool lds_add(u64 *lkey, unsigned *lcount, u64 key, unsigned count)
{
  unsigned i = (unsigned)mix(key) & (kLds - 1);
  for (unsigned probe = 0; probe < kLdsProbe; ++probe, i = (i + 1) & (kLds - 1)) {
    u64 cur = __hip_atomic_load(lkey + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == kEmpty &&
        __hip_atomic_compare_exchange_strong(lkey + i, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
      cur = key;
    if (cur == key) { __hip_atomic_fetch_add(lcount + i, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); return true; }
  }
  return false;
}

// src the parent words of the numbered forest, src2 the plane B, dst the member's slots (cleared by the host), src_stride their number,
// sums the member's four control words (zeroed); h2 != 0: the member sits this launch out (its table was large enough)
__global__ void __launch_bounds__(CVH_BLOCK) overlap_pairs_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ u64 lkey[kLds];
  __shared__ unsigned lcount[kLds];
  const CvhIoMember *m = tab + overlap_member(tab, nmem);
  if (m->h2) return;   // (the same for the whole workgroup)
  for (unsigned s = threadIdx.x; s < kLds; s += CVH_BLOCK) { lkey[s] = kEmpty; lcount[s] = 0; }
  __syncthreads();
  const unsigned n = (unsigned)m->n;   // (h w < 2^31)
  const gwords parent = (gwords)m->src;
  CVH_GLOBAL const int *other = (CVH_GLOBAL const int *)m->src2;
  CVH_GLOBAL CvhOverlapSlot *slots = (CVH_GLOBAL CvhOverlapSlot *)m->dst;
  CVH_GLOBAL unsigned *ctl = (CVH_GLOBAL unsigned *)m->sums;
  const u64 nslots = m->src_stride;
  const u64 tile0 = (u64)(blockIdx.x - m->first) * CVH_MEASURE_TILE;
  const unsigned lane = lane_id();
  for (unsigned t = 0; t < CVH_MEASURE_TILE; t += CVH_BLOCK) {
    if (tile0 + t >= n) break;
    const u64 q = tile0 + t + threadIdx.x;
    const bool live = q < n;
    const unsigned p = live ? (unsigned)q : 0u;
    const unsigned a = live ? label_of(parent, p) : 0u, b = live ? (unsigned)other[p] : 0u;
    // the runs of the wave: a run starts where the key changes (a row end inside a run changes no count)
    const unsigned pa = __shfl_up(a, 1, 64), pb = __shfl_up(b, 1, 64);
    const bool start = live && (lane == 0 || pa != a || pb != b);
    const u64 ends = __ballot(start || !live) & ~upto(lane);
    if (!start) continue;
    const unsigned count = (ends ? (unsigned)__builtin_ctzll(ends) : 64u) - lane;
    const u64 key = ((u64)(a + 1u) << 32) | b;
    if (!lds_add(lkey, lcount, key, count)) global_add(slots, nslots, ctl, key, count);
  }
  __syncthreads();
  for (unsigned s = threadIdx.x; s < kLds; s += CVH_BLOCK)
    if (lkey[s] != kEmpty) global_add(slots, nslots, ctl, lkey[s], lcount[s]);
}

// the occupied slots of every member, compacted into plane[0] (slots / 2 rows: what a table that did not overflow can hold) in the
// order the waves arrive -- the host sorts; ctl[2] counts them.  A wave takes one position for all its rows (ballot, one atomic).
__global__ void __launch_bounds__(CVH_BLOCK) overlap_rows_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + overlap_member(tab, nmem);
  CVH_GLOBAL unsigned *ctl = (CVH_GLOBAL unsigned *)m->sums;
  if (m->h2 || !m->w2 || DEV_LOAD(ctl + 1)) return;   // sits out, no rows asked for, or overflowed: the same for the whole workgroup
  CVH_GLOBAL const CvhOverlapSlot *slots = (CVH_GLOBAL const CvhOverlapSlot *)m->dst;
  CVH_GLOBAL cvh_overlap *rows = (CVH_GLOBAL cvh_overlap *)m->plane[0];
  const u64 nslots = m->src_stride, cap = nslots / 2, stride = (u64)m->nblk * CVH_BLOCK;
  const unsigned lane = lane_id();
  for (u64 base = (u64)(blockIdx.x - m->first) * CVH_BLOCK + (threadIdx.x & ~63u); base < nslots; base += stride) {   // (per wave)
    const u64 s = base + lane;
    const u64 key = s < nslots ? slots[s].key : kEmpty;
    const u64 bits = __ballot(key != kEmpty);
    if (!bits) continue;
    unsigned pos = 0;
    if (lane == (unsigned)__builtin_ctzll(bits)) pos = DEV_ADD(ctl + 2, (unsigned)__builtin_popcountll(bits));
    pos = __shfl(pos, __builtin_ctzll(bits), 64) + (unsigned)__builtin_popcountll(bits & (upto(lane) >> 1));
    if (key != kEmpty && pos < cap) {
      rows[pos].a = (int)(unsigned)(key >> 32) - 1; rows[pos].b = (int)(unsigned)key;
      rows[pos].count = slots[s].count; rows[pos].pad = 0;
    }
  }
}

}  // namespace

// behind the numbering launches (cvh_launch_cc_number): the pairs of every member that does not sit out, and with any_rows their rows
hipError_t cvh_launch_overlap(const CvhIoMember *tab, int nmem, unsigned grid, bool any_rows, hipStream_t s)
{
  hipLaunchKernelGGL(overlap_pairs_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  if (any_rows) hipLaunchKernelGGL(overlap_rows_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}
