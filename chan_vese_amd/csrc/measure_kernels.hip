// measure_kernels.hip — the rows of cvh_measure* (include/chanvese_hip.h, "Component measures"; gfx950): per component of a NUMBERED forest
// (components_kernels.hip, behind cc_number_kernel) its area, box, border count, perimeter, coordinate moments and intensity sums.  All
// integers, all sums: neither the grid, the schedule nor the cache below can change a bit of a row.
// A member's section is ceil(h w / CVH_MEASURE_TILE) workgroups; a workgroup makes CVH_MEASURE_TILE / 256 trips over its tile in flat
// raster order, so a wave holds 64 consecutive flat indices per trip (as the components kernels).  Per trip a lane
//   reads its label (parent word, and the root's word where the pixel is no root), the class of its four neighbours (left and right from the
//   wave's ballot, the wave's two end lanes and up / down from the parent words) and its C image bytes;
//   a SEGMENTED suffix sum over the horizontal run inside the wave (six steps of __shfl_down, 32-bit partials: a run has at most 64 pixels, so
//   perimeter <= 256, border <= 64, sum I <= 16320, sum I^2 <= 4161600) leaves the run's sums in the run's first lane;
//   that lane adds the closed forms of (row, first column, length) for area, box and the five coordinate sums -- 64-bit from here on.
// AGGREGATION.  The workgroup keeps kSlots rows in LDS, direct-mapped by label.  Per trip, between workgroup barriers:
//   A  a run whose slot is empty or holds its label adds there (LDS atomics: 64-bit adds, 32-bit min / max);
//   B  of the runs that found another label in their slot ONE per slot (an LDS atomic max of the trip number picks it) sends the resident row to the
//      global row with 64-bit atomics -- the eviction -- and puts its own sums in its place; the others of that slot and trip add to
//      their global rows directly.
// After the last trip every occupied slot goes out once.  A plane that is one component therefore sends one set of global atomics per
// WORKGROUP, not per run.  Nothing here waits for or polls another workgroup.
#include <limits.h>

#include "cvh_internal.h"

namespace {

#define CVH_GLOBAL __attribute__((address_space(1)))
typedef CVH_GLOBAL const unsigned *gwords;
typedef unsigned long long u64;

static_assert(CVH_BLOCK == 256 && CVH_MEASURE_TILE % CVH_BLOCK == 0, "a trip is four waves of 64 consecutive pixels");
// components_kernels.hip's encoding of the parent words behind cc_number_kernel
constexpr unsigned kNone = 0xffffffffu;       // not a pixel of the class
constexpr unsigned kNumbered = 0x80000000u;   // a root: kNumbered | k, k = 1 .. K; every other pixel of the class holds its root's index
constexpr int kSlots = 64, kSums = 12;        // rows in LDS; the 64-bit sums of a row: perimeter, sx, sy, sxx, syy, sxy, s1[3], s2[3]
constexpr unsigned kEmpty = 0;                // (labels start at 1)

__device__ __forceinline__ int measure_member(const CvhIoMember *tab, int nmem)
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

// what a run adds to its row
struct Run {
  unsigned area, border; int x0, y0, x1, y1;
  u64 s[kSums];
};

struct Slot {   // 128 bytes
  unsigned key, claim, area, border; int x0, y0, x1, y1;
  u64 s[kSums];
};

__device__ __forceinline__ void slot_clear(Slot *q)
{
  q->key = kEmpty; q->claim = 0; q->area = 0; q->border = 0;
  q->x0 = INT_MAX; q->y0 = INT_MAX; q->x1 = -1; q->y1 = -1;
  for (int i = 0; i < kSums; ++i) q->s[i] = 0;
}

#define LDS_ADD(P, V) __hip_atomic_fetch_add((P), (V), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define DEV_ADD(P, V) __hip_atomic_fetch_add((P), (V), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ __forceinline__ void slot_add(Slot *q, const Run &a)
{
  LDS_ADD(&q->area, a.area);
  if (a.border) LDS_ADD(&q->border, a.border);
  __hip_atomic_fetch_min(&q->x0, a.x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_min(&q->y0, a.y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_max(&q->x1, a.x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_max(&q->y1, a.y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  for (int i = 0; i < kSums; ++i)
    if (a.s[i]) LDS_ADD(&q->s[i], a.s[i]);
}

// the global row of label k takes what a run or a slot holds: adds of zero are left out, min and max go out only where they would move the value
__device__ __forceinline__ void row_add(CVH_GLOBAL cvh_region *row, unsigned area, unsigned border, int x0, int y0, int x1, int y1, const u64 *s)
{
  DEV_ADD(&row->area, area);
  if (border) DEV_ADD(&row->border, border);
  if (x0 < __hip_atomic_load(&row->x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_min(&row->x0, x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (y0 < __hip_atomic_load(&row->y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_min(&row->y0, y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (x1 > __hip_atomic_load(&row->x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_max(&row->x1, x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (y1 > __hip_atomic_load(&row->y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_fetch_max(&row->y1, y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  CVH_GLOBAL u64 *sums = (CVH_GLOBAL u64 *)&row->perimeter;   // perimeter, sx, sy, sxx, syy, sxy, s1[3], s2[3]: twelve words in a row
  for (int i = 0; i < kSums; ++i)
    if (s[i]) DEV_ADD(sums + i, s[i]);
}

// the label of pixel p (0 outside the class)
__device__ __forceinline__ unsigned label_of(gwords parent, unsigned p)
{
  const unsigned v = parent[p];
  if (v == kNone) return 0;
  return ((v & kNumbered) ? v : parent[v]) & ~kNumbered;
}

// v summed from this lane to the last lane of its run (lanes lane .. end - 1)
__device__ __forceinline__ unsigned run_suffix_sum(unsigned v, unsigned end)
{
  const unsigned lane = lane_id();
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_down(v, d, 64);
    if (lane + d < end) v += o;
  }
  return v;
}

// the roots whose rows the table holds write `first` and the neutral elements (the rows are the member's dst, `rows` of them)
__global__ void __launch_bounds__(CVH_BLOCK) measure_init_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + measure_member(tab, nmem);
  const unsigned n = (unsigned)m->n, rows = (unsigned)m->h2;   // (h w < 2^31)
  const gwords parent = (gwords)m->src;
  const u64 tile0 = (u64)(blockIdx.x - m->first) * CVH_MEASURE_TILE;
  for (unsigned t = 0; t < CVH_MEASURE_TILE; t += CVH_BLOCK) {
    const u64 q = tile0 + t + threadIdx.x;
    if (q >= n) break;
    const unsigned p = (unsigned)q, v = parent[p];
    if (v == kNone || !(v & kNumbered) || (v & ~kNumbered) - 1u >= rows) continue;
    CVH_GLOBAL cvh_region *row = (CVH_GLOBAL cvh_region *)m->dst + ((v & ~kNumbered) - 1u);
    row->first = p; row->area = 0;
    row->x0 = INT_MAX; row->y0 = INT_MAX; row->x1 = -1; row->y1 = -1;
    row->border = 0; row->reserved = 0;
    CVH_GLOBAL u64 *sums = (CVH_GLOBAL u64 *)&row->perimeter;
    for (int i = 0; i < kSums; ++i) sums[i] = 0;
  }
}

template <int C>
__device__ __forceinline__ void measure_tile(const CvhIoMember *m, Slot *slot)
{
  const unsigned n = (unsigned)m->n, w = (unsigned)m->w, h = (unsigned)m->h, rows = (unsigned)m->h2;
  const gwords parent = (gwords)m->src;
  CVH_GLOBAL cvh_region *table = (CVH_GLOBAL cvh_region *)m->dst;
  const u64 tile0 = (u64)(blockIdx.x - m->first) * CVH_MEASURE_TILE;
  const unsigned lane = lane_id();

  for (unsigned t = 0; t < CVH_MEASURE_TILE; t += CVH_BLOCK) {
    if (tile0 + t >= n) break;   // (the same for every lane of the workgroup: the barriers below stay whole)
    const u64 q = tile0 + t + threadIdx.x;
    const bool live = q < n;
    const unsigned p = live ? (unsigned)q : 0u;
    const unsigned k = live ? label_of(parent, p) : 0u;
    const unsigned r = p / w, c = p - r * w;
    const u64 bits = __ballot(k != 0);
    unsigned pb = 0, s1a = 0, s1b = 0, s2[C];
#pragma unroll
    for (int j = 0; j < C; ++j) s2[j] = 0;
    if (k) {
      const bool left = c > 0 && (lane > 0 ? ((bits >> (lane - 1)) & 1ull) != 0 : parent[p - 1] != kNone);
      const bool right = c + 1 < w && (lane < 63 ? ((bits >> (lane + 1)) & 1ull) != 0 : parent[p + 1] != kNone);
      const bool up = r > 0 && parent[p - w] != kNone, down = r + 1 < h && parent[p + w] != kNone;
      const unsigned edges = 4u - (left ? 1u : 0u) - (right ? 1u : 0u) - (up ? 1u : 0u) - (down ? 1u : 0u);
      const unsigned on_border = (r == 0 || r == h - 1 || c == 0 || c == w - 1) ? 1u : 0u;
      pb = edges | (on_border << 16);   // two counts in one word: a run has at most 256 edges and 64 border pixels
#pragma unroll
      for (int j = 0; j < C; ++j) {
        const unsigned v = ((CVH_GLOBAL const uint8_t *)m->plane[j])[p];
        if (j == 0) s1a = v; else if (j == 1) s1a |= v << 16; else s1b = v;   // (a run's sum I is at most 16320: 16 bits each)
        s2[j] = v * v;
      }
    }
    // the runs of the wave: a run starts where the label changes or a row of the plane begins
    const unsigned key = k ? k : kNone, prev = __shfl_up(key, 1, 64);
    const bool start = k != 0 && (lane == 0 || prev != key || c == 0);
    const u64 ends = __ballot(start || k == 0) & ~upto(lane);
    const unsigned end = ends ? (unsigned)__builtin_ctzll(ends) : 64u;
    pb = run_suffix_sum(pb, end);
    s1a = run_suffix_sum(s1a, end);
    if (C > 2) s1b = run_suffix_sum(s1b, end);
#pragma unroll
    for (int j = 0; j < C; ++j) s2[j] = run_suffix_sum(s2[j], end);

    const bool mine = start && k - 1u < rows;   // (a label beyond the rows the caller asked for has no row)
    Run a;
    bool miss = false;
    Slot *q_slot = slot + (k & (kSlots - 1));
    if (mine) {
      const u64 L = end - lane, c0 = c, row = r;
      a.area = (unsigned)L; a.border = pb >> 16;
      a.x0 = (int)c; a.x1 = (int)(c + (unsigned)L - 1u); a.y0 = (int)r; a.y1 = (int)r;
      const u64 tri = L * (L - 1) / 2, sx = L * c0 + tri;
      a.s[0] = pb & 0xffffu;
      a.s[1] = sx;
      a.s[2] = row * L;
      a.s[3] = L * c0 * c0 + 2 * c0 * tri + (L - 1) * L * (2 * L - 1) / 6;
      a.s[4] = row * row * L;
      a.s[5] = row * sx;
      a.s[6] = s1a & 0xffffu; a.s[7] = C > 1 ? s1a >> 16 : 0u; a.s[8] = C > 2 ? s1b : 0u;
#pragma unroll
      for (int j = 0; j < 3; ++j) a.s[9 + j] = j < C ? s2[j < C ? j : 0] : 0u;
      // A: the slot is empty (and now this label's) or this label's already
      unsigned seen = kEmpty;
      const bool ok = __hip_atomic_compare_exchange_strong(&q_slot->key, &seen, k, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (ok || seen == k) slot_add(q_slot, a); else miss = true;
    }
    __syncthreads();
    // B: nobody adds to a slot now.  One of the runs that met another label evicts it; the others go out directly
    if (miss) {
      const unsigned trip = t / CVH_BLOCK + 1u;   // the slot's claim word holds the last trip that evicted it: no lane has to clear it
      if (__hip_atomic_fetch_max(&q_slot->claim, trip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < trip) {
        row_add(table + (q_slot->key - 1u), q_slot->area, q_slot->border, q_slot->x0, q_slot->y0, q_slot->x1, q_slot->y1, q_slot->s);
        q_slot->key = k; q_slot->area = a.area; q_slot->border = a.border;
        q_slot->x0 = a.x0; q_slot->y0 = a.y0; q_slot->x1 = a.x1; q_slot->y1 = a.y1;
        for (int i = 0; i < kSums; ++i) q_slot->s[i] = a.s[i];
      } else {
        row_add(table + (k - 1u), a.area, a.border, a.x0, a.y0, a.x1, a.y1, a.s);
      }
    }
    __syncthreads();
  }
}

template <int C>
__global__ void __launch_bounds__(CVH_BLOCK) measure_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ Slot slot[kSlots];
  const CvhIoMember *m = tab + measure_member(tab, nmem);
  if (m->C != C || !m->h2) return;   // (the other instantiation's member, or a member without rows: the same for the whole workgroup)
  if (threadIdx.x < kSlots) slot_clear(slot + threadIdx.x);
  __syncthreads();
  measure_tile<C>(m, slot);
  // (the loop's last barrier is behind every add)
  if (threadIdx.x < kSlots && slot[threadIdx.x].key != kEmpty) {
    const Slot *q = slot + threadIdx.x;
    row_add((CVH_GLOBAL cvh_region *)m->dst + (q->key - 1u), q->area, q->border, q->x0, q->y0, q->x1, q->y1, q->s);
  }
}

}  // namespace

unsigned cvh_measure_blocks(size_t n) { return (unsigned)((n + CVH_MEASURE_TILE - 1) / CVH_MEASURE_TILE); }

// behind the numbering launches (cvh_launch_cc_number): the rows of every member's table
hipError_t cvh_launch_measure(const CvhIoMember *tab, int nmem, unsigned grid, bool any_c1, bool any_c3, hipStream_t s)
{
  hipLaunchKernelGGL(measure_init_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  if (any_c1) hipLaunchKernelGGL(measure_kernel<1>, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  if (any_c3) hipLaunchKernelGGL(measure_kernel<3>, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}
