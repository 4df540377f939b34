// contour_kernels.hip — the boundary of the mask as ordered closed loops (cvh_contours*; include/chanvese_hip.h, "Contours"; gfx950).
// Everything is integers; the launches are ordered by their kernel boundaries alone -- no workgroup waits for or polls another, no
// cooperative launch -- and each is ONE grid over N members of mixed shapes (CvhIoMember, sections first / nblk).
// A member's entry:  src the mask bytes, plane[0] the 4-bit edge sets (a byte per pixel), plane[1] a word per pixel (the number of
// edges before the pixel: inside its workgroup after the bits launch, inside the member after the link launch), plane[2] a count per
// 256 pixels -- the context's per-pixel workspace --; dst the per-edge workspace of src_stride edges (EdgeSpace below); src2 the point
// array (int32 x, y; may be null), h2 / w2 the low / high half of the point cap; sums the member's words {E, loops, points}.
//   PIXEL launches (a lane per pixel, cvh_cc_blocks(n) workgroups):  bits.   Then a one-wave scan per member: E.   -- host wait: E --
//   EDGE launches (cvh_contour_edge_blocks(E, n) workgroups, a lane takes edge or pixel i, i + 256 nblk, ...):
//     link      per pixel: the compact index of each of its edges (monotone in the edge id), the edge's id, its successor, its weight
//     double    R rounds, double-buffered: after round r an edge holds {succ^(2^r), the minimum index in the 2^r edges from it, the
//               weight in front of that minimum's FIRST occurrence, the weight of the 2^r edges}; 2^R >= E covers every cycle
//     heads     the edges that are their cycle's minimum, counted per 256 edges; scan: the loop index of the heads and the loop count
//     rows      a head writes its loop's row (first; the sums zero) and keeps its loop index where the idle buffer is
//     sums      edges, points and area2 per loop: runs of one loop inside a wave are combined first (ballots, a segmented 64-bit
//               reduction), one set of 64-bit / 32-bit vector atomics per run -- a plane that is one loop sends one set per wave
//     offsets   points summed per 256 loops, scan, then the exclusive prefix: offset; the point count
//     scatter   every (corner) edge writes its tail vertex at offset + (points - weight in front of the head) mod points -- or, for
//               cvh_contours_subpixel* (every edge a point), the zero level's crossing of the edge at that place: two doubles, gathered
//               from the level set (the ONE use of floating point here; the member's src2 is then double x, y)
#include "cvh_internal.h"

namespace {

#define CVH_GLOBAL __attribute__((address_space(1)))
typedef CVH_GLOBAL unsigned *gwords;
typedef unsigned quad __attribute__((ext_vector_type(4)));   // one 16-byte load or store
typedef CVH_GLOBAL quad *gquads;
__device__ __forceinline__ quad make_quad(unsigned x, unsigned y, unsigned z, unsigned w) { quad q = {x, y, z, w}; return q; }
typedef CVH_GLOBAL const uint8_t *gbytes;
typedef double point2 __attribute__((ext_vector_type(2), aligned(8)));   // a subpixel point, x then y: one 16-byte store to an 8-byte aligned place

static_assert(CVH_BLOCK == 256, "the per-wave counts below are summed as four waves");
static_assert(sizeof(cvh_contour_loop) == 32, "a loop row is 32 bytes");

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ unsigned long long below(unsigned lane) { return (1ull << lane) - 1ull; }   // bits 0 .. lane - 1

// the member whose section holds this workgroup (components_kernels.hip's cc_member); members without edges have empty sections
__device__ __forceinline__ const CvhIoMember *section(const CvhIoMember *tab, int nmem)
{
  int lo = 0, hi = nmem - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return tab + lo;
}

// the per-edge workspace of a member with room for cap edges (cvh_contour_edge_bytes)
struct EdgeSpace {
  gquads buf[2];     // {succ, min, weight in front of min, weight}: the doubling's two buffers
  gwords id;         // edge id of compact index e
  gwords heads;      // heads per 256 edges, then their exclusive scan
  gwords lsum;       // points per 256 loops, then their exclusive scan
  CVH_GLOBAL uint8_t *corner;   // the weight of the edge: 1 where its tail vertex is a point of the loop
  CVH_GLOBAL cvh_contour_loop *rows;
};
__host__ __device__ constexpr size_t edge_chunks(size_t cap) { return (cap + CVH_BLOCK - 1) / CVH_BLOCK; }
__host__ __device__ constexpr size_t edge_rows(size_t cap) { return cap / 4 + 1; }   // (a cycle has at least four edges)
__device__ __forceinline__ EdgeSpace edge_space(const CvhIoMember *m)
{
  const size_t cap = (size_t)m->src_stride;
  EdgeSpace s;
  uint8_t *p = (uint8_t *)m->dst;
  s.buf[0] = (gquads)p; p += cap * sizeof(quad);
  s.buf[1] = (gquads)p; p += cap * sizeof(quad);
  s.rows = (CVH_GLOBAL cvh_contour_loop *)p; p += edge_rows(cap) * sizeof(cvh_contour_loop);
  s.id = (gwords)p; p += cap * sizeof(unsigned);
  s.heads = (gwords)p; p += edge_chunks(cap) * sizeof(unsigned);
  s.lsum = (gwords)p; p += edge_chunks(edge_rows(cap)) * sizeof(unsigned);
  s.corner = (CVH_GLOBAL uint8_t *)p;
  return s;
}
__device__ __forceinline__ unsigned edges_of(const CvhIoMember *m) { return (unsigned)m->sums[0]; }

// inclusive sum over the lanes of a wave
__device__ __forceinline__ unsigned wave_scan(unsigned v)
{
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl_up(v, d, 64);
    if (lane_id() >= d) v += t;
  }
  return v;
}

// the sum of v over the lanes of the workgroup before this one; *total: over all of them.  part: four words of LDS, free again behind
// the call (two barriers)
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned *part, unsigned *total)
{
  const unsigned incl = wave_scan(v), wave = threadIdx.x >> 6;
  if (lane_id() == 63) part[wave] = incl;
  __syncthreads();
  const unsigned p0 = part[0], p1 = part[1], p2 = part[2], p3 = part[3];
  __syncthreads();
  *total = p0 + p1 + p2 + p3;
  return incl - v + (wave > 0 ? p0 : 0u) + (wave > 1 ? p1 : 0u) + (wave > 2 ? p2 : 0u);
}

// is (r, c) a foreground pixel of the member's mask; outside the plane: no
__device__ __forceinline__ bool fg(gbytes mask, int h, int w, int r, int c)
{
  return r >= 0 && r < h && c >= 0 && c < w && mask[(size_t)r * (unsigned)w + (unsigned)c] != 0;
}

// direction k (0 east, 1 south, 2 west, 3 north; y grows downwards): the step forward and the step to the right, as (rows, columns)
__device__ __forceinline__ void steps(unsigned k, int *fr, int *fc, int *rr, int *rc)
{
  *fr = k == 1 ? 1 : (k == 3 ? -1 : 0);
  *fc = k == 0 ? 1 : (k == 2 ? -1 : 0);
  *rr = *fc; *rc = -*fr;   // east -> south, south -> west, west -> north, north -> east
}

// the tail vertex of edge k of pixel (r, c)
__device__ __forceinline__ void tail_of(unsigned k, int r, int c, int *x, int *y)
{
  *x = c + (k == 1 || k == 2 ? 1 : 0);
  *y = r + (k >= 2 ? 1 : 0);
}

// PIXEL launch: the boundary edges of every pixel, counted per workgroup
__global__ void __launch_bounds__(CVH_BLOCK) contour_bits_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned part[CVH_BLOCK / 64];
  const CvhIoMember *m = section(tab, nmem);
  const unsigned n = (unsigned)m->n, p = (blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x;   // (h w < 2^30)
  const gbytes mask = (gbytes)m->src;
  unsigned bits = 0;
  if (p < n && mask[p]) {
    const int h = m->h, w = m->w, r = (int)(p / (unsigned)w), c = (int)(p % (unsigned)w);
    bits = (fg(mask, h, w, r - 1, c) ? 0u : 1u) | (fg(mask, h, w, r, c + 1) ? 0u : 2u) | (fg(mask, h, w, r + 1, c) ? 0u : 4u) |
           (fg(mask, h, w, r, c - 1) ? 0u : 8u);
  }
  unsigned total;
  const unsigned before = block_scan((unsigned)__builtin_popcount(bits), part, &total);
  if (p < n) {
    ((CVH_GLOBAL uint8_t *)m->plane[0])[p] = (uint8_t)bits;
    ((gwords)m->plane[1])[p] = before;
  }
  if (threadIdx.x == 0) ((gwords)m->plane[2])[blockIdx.x - m->first] = total;
}

// ONE wave per member: nb counts become their exclusive prefix sums, 64 per trip; the total goes to the member's word `word`.
// what 0: the edges per 256 pixels (E), 1: the heads per 256 edges (loops), 2: the points per 256 loops (points)
__global__ void __launch_bounds__(64) contour_scan_kernel(const CvhIoMember *tab, int nmem, int what)
{
  const CvhIoMember *m = tab + blockIdx.x;
  gwords cnt;
  unsigned nb;
  if (what == 0) {
    cnt = (gwords)m->plane[2];
    nb = ((unsigned)m->n + CVH_BLOCK - 1) / CVH_BLOCK;
  } else {
    const unsigned items = what == 1 ? edges_of(m) : (unsigned)m->sums[1];
    if (!items) return;   // (no edge workspace: the member's words stay zero)
    const EdgeSpace s = edge_space(m);
    cnt = what == 1 ? s.heads : s.lsum;
    nb = (items + CVH_BLOCK - 1) / CVH_BLOCK;
  }
  unsigned carry = 0, v = threadIdx.x < nb ? cnt[threadIdx.x] : 0u;
  for (unsigned i = threadIdx.x; i - threadIdx.x < nb; i += 64) {
    const unsigned next = i + 64 < nb ? cnt[i + 64] : 0u;   // (in flight while this trip's counts are scanned)
    const unsigned incl = wave_scan(v);
    if (i < nb) cnt[i] = carry + incl - v;
    carry += __shfl(incl, 63, 64);
    v = next;
  }
  if (threadIdx.x == 0) m->sums[what] = carry;
}

// EDGE launch, over the PIXELS: the prefix of a pixel becomes the member-wide one; its edges take their compact indices
__global__ void __launch_bounds__(CVH_BLOCK) contour_prefix_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = section(tab, nmem);
  const unsigned n = (unsigned)m->n, stride = m->nblk * CVH_BLOCK;
  const gwords pre = (gwords)m->plane[1], cnt = (gwords)m->plane[2];
  for (unsigned p = (blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x; p < n; p += stride) pre[p] += cnt[p / CVH_BLOCK];
}

// the compact index of edge k of pixel q (a boundary edge)
__device__ __forceinline__ unsigned compact(gwords pre, gbytes bits, unsigned q, unsigned k)
{
  return pre[q] + (unsigned)__builtin_popcount((unsigned)bits[q] & ((1u << k) - 1u));
}

// EDGE launch, over the PIXELS: id, successor and weight of every edge -- round 0 of the doubling
__global__ void __launch_bounds__(CVH_BLOCK) contour_link_kernel(const CvhIoMember *tab, int nmem, int conn, int simplify)
{
  const CvhIoMember *m = section(tab, nmem);
  const unsigned n = (unsigned)m->n, stride = m->nblk * CVH_BLOCK;
  const int h = m->h, w = m->w;
  const gbytes mask = (gbytes)m->src, bits = (gbytes)m->plane[0];
  const gwords pre = (gwords)m->plane[1];
  const EdgeSpace s = edge_space(m);
  for (unsigned p = (blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x; p < n; p += stride) {
    const unsigned b = bits[p];
    if (!b) continue;
    const int r = (int)(p / (unsigned)w), c = (int)(p % (unsigned)w);
    unsigned e = pre[p];
    for (unsigned k = 0; k < 4; ++k) {
      if (!(b >> k & 1u)) continue;
      int fr, fc, rr, rc;
      steps(k, &fr, &fc, &rr, &rc);
      // at the head: the pixel in front (on the right of the edge continued) and the one in front on the left
      const bool front = fg(mask, h, w, r + fr, c + fc), front_left = fg(mask, h, w, r + fr - rr, c + fc - rc);
      unsigned next;
      if (front_left && (front || conn == 8)) next = compact(pre, bits, (unsigned)((r + fr - rr) * w + (c + fc - rc)), (k + 3u) & 3u);   // left turn
      else if (front) next = compact(pre, bits, (unsigned)((r + fr) * w + (c + fc)), k);                                                 // straight on
      else next = e - (unsigned)__builtin_popcount(b & ((1u << k) - 1u)) + (unsigned)__builtin_popcount(b & ((1u << ((k + 1u) & 3u)) - 1u));   // right turn: the pixel's own next side
      // at the tail: the predecessor runs straight on exactly where the pixel behind is foreground and the one behind on the left
      // does not take the turn
      const bool back = fg(mask, h, w, r - fr, c - fc), back_left = fg(mask, h, w, r - fr - rr, c - fc - rc);
      const bool straight = back && !(back_left && (back || conn == 8));
      const unsigned weight = simplify && straight ? 0u : 1u;
      s.id[e] = 4u * p + k;
      s.corner[e] = (uint8_t)weight;
      s.buf[0][e] = make_quad(next, e, 0u, weight);
      ++e;
    }
  }
}

// one round: windows of 2^r edges become windows of 2^(r+1).  Ties keep the nearer minimum (a window may go round its cycle)
__global__ void __launch_bounds__(CVH_BLOCK) contour_double_kernel(const CvhIoMember *tab, int nmem, int from)
{
  const CvhIoMember *m = section(tab, nmem);
  const unsigned E = edges_of(m), stride = m->nblk * CVH_BLOCK;
  const EdgeSpace s = edge_space(m);
  const gquads in = s.buf[from], out = s.buf[from ^ 1];
  for (unsigned e = (blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x; e < E; e += stride) {
    const quad a = in[e], b = in[a.x];
    out[e] = make_quad(b.x, b.y < a.y ? b.y : a.y, b.y < a.y ? a.w + b.z : a.z, a.w + b.w);
  }
}

// the heads (an edge that is its cycle's minimum), counted per 256 edges
__global__ void __launch_bounds__(CVH_BLOCK) contour_heads_kernel(const CvhIoMember *tab, int nmem, int res)
{
  __shared__ unsigned part[CVH_BLOCK / 64];
  const CvhIoMember *m = section(tab, nmem);
  const unsigned E = edges_of(m), chunks = (E + CVH_BLOCK - 1) / CVH_BLOCK;
  const EdgeSpace s = edge_space(m);
  for (unsigned chunk = blockIdx.x - m->first; chunk < chunks; chunk += m->nblk) {
    const unsigned e = chunk * CVH_BLOCK + threadIdx.x;
    const unsigned long long heads = __ballot(e < E && s.buf[res][e].y == e);
    if (lane_id() == 0) part[threadIdx.x >> 6] = (unsigned)__builtin_popcountll(heads);
    __syncthreads();
    if (threadIdx.x == 0) s.heads[chunk] = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
  }
}

// a head takes its loop index (loops are numbered by their smallest edge), opens its row and leaves the index in the idle buffer
__global__ void __launch_bounds__(CVH_BLOCK) contour_rows_kernel(const CvhIoMember *tab, int nmem, int res)
{
  __shared__ unsigned part[CVH_BLOCK / 64];
  const CvhIoMember *m = section(tab, nmem);
  const unsigned E = edges_of(m), chunks = (E + CVH_BLOCK - 1) / CVH_BLOCK;
  const EdgeSpace s = edge_space(m);
  for (unsigned chunk = blockIdx.x - m->first; chunk < chunks; chunk += m->nblk) {
    const unsigned e = chunk * CVH_BLOCK + threadIdx.x;
    const bool head = e < E && s.buf[res][e].y == e;
    unsigned total;
    const unsigned k = s.heads[chunk] + block_scan(head ? 1u : 0u, part, &total);
    if (!head) continue;
    ((gwords)(s.buf[res ^ 1] + e))[0] = k;
    CVH_GLOBAL quad *row = (CVH_GLOBAL quad *)(s.rows + k);
    row[0] = make_quad(s.id[e], 0u, 0u, 0u);   // first, edges, points, pad
    row[1] = make_quad(0u, 0u, 0u, 0u);        // offset, area2
  }
}

// edges, points and area2 of every loop
__global__ void __launch_bounds__(CVH_BLOCK) contour_sums_kernel(const CvhIoMember *tab, int nmem, int res)
{
  const CvhIoMember *m = section(tab, nmem);
  const unsigned E = edges_of(m), stride = m->nblk * CVH_BLOCK, w = (unsigned)m->w;
  const EdgeSpace s = edge_space(m);
  const unsigned lane = lane_id();
  for (unsigned e0 = (blockIdx.x - m->first) * CVH_BLOCK + (threadIdx.x & ~63u); e0 < E; e0 += stride) {   // (wave-uniform trips)
    const unsigned e = e0 + lane;
    const bool live = e < E;
    unsigned loop = 0xffffffffu, corner = 0;
    long long cross = 0;
    if (live) {
      const quad a = s.buf[res][e];
      loop = ((gwords)(s.buf[res ^ 1] + a.y))[0];   // (a.y is a head: the minimum of a cycle is its own minimum)
      corner = s.corner[e];
      const unsigned id = s.id[e], k = id & 3u, p = id >> 2;
      int x, y, fr, fc, rr, rc;
      tail_of(k, (int)(p / w), (int)(p % w), &x, &y);
      steps(k, &fr, &fc, &rr, &rc);
      cross = (long long)x * (y + fr) - (long long)(x + fc) * y;
    }
    // runs of one loop over neighbouring lanes: numbered, so that equal numbers d lanes apart mean one run
    const unsigned prev = __shfl_up(loop, 1, 64);
    const bool start = live && loop < (unsigned)m->sums[1] && (lane == 0 || prev != loop);   // (never a row that does not exist)
    const unsigned long long starts = __ballot(start), lives = __ballot(live);
    const unsigned run = (unsigned)__builtin_popcountll(starts & (below(lane) | (1ull << lane)));
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
      const long long other = __shfl_down(cross, d, 64);
      const unsigned other_run = __shfl_down(run, d, 64);
      if (lane + d < 64 && other_run == run && (lives >> (lane + d) & 1ull)) cross += other;
    }
    const unsigned long long corners = __ballot(corner != 0);
    if (!start) continue;
    const unsigned long long later = starts & ~(below(lane) | (1ull << lane));
    const unsigned end = later ? (unsigned)__builtin_ctzll(later) : 64u;   // the run is lanes lane .. end - 1 (of the live ones)
    const unsigned long long mine = lives & (end == 64 ? ~0ull : below(end)) & ~below(lane);
    CVH_GLOBAL cvh_contour_loop *row = s.rows + loop;
    __hip_atomic_fetch_add(&row->edges, (unsigned)__builtin_popcountll(mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned pts = (unsigned)__builtin_popcountll(mine & corners);
    if (pts) __hip_atomic_fetch_add(&row->points, pts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cross) __hip_atomic_fetch_add((CVH_GLOBAL unsigned long long *)&row->area2, (unsigned long long)cross, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the points of every 256 loops
__global__ void __launch_bounds__(CVH_BLOCK) contour_loop_sums_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned part[CVH_BLOCK / 64];
  const CvhIoMember *m = section(tab, nmem);
  const unsigned L = (unsigned)m->sums[1], chunks = (L + CVH_BLOCK - 1) / CVH_BLOCK;
  const EdgeSpace s = edge_space(m);
  for (unsigned chunk = blockIdx.x - m->first; chunk < chunks; chunk += m->nblk) {
    const unsigned k = chunk * CVH_BLOCK + threadIdx.x;
    unsigned total;
    (void)block_scan(k < L ? s.rows[k].points : 0u, part, &total);
    if (threadIdx.x == 0) s.lsum[chunk] = total;
  }
}

// offset = the points of the loops before
__global__ void __launch_bounds__(CVH_BLOCK) contour_offsets_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned part[CVH_BLOCK / 64];
  const CvhIoMember *m = section(tab, nmem);
  const unsigned L = (unsigned)m->sums[1], chunks = (L + CVH_BLOCK - 1) / CVH_BLOCK;
  const EdgeSpace s = edge_space(m);
  for (unsigned chunk = blockIdx.x - m->first; chunk < chunks; chunk += m->nblk) {
    const unsigned k = chunk * CVH_BLOCK + threadIdx.x;
    unsigned total;
    const unsigned before = s.lsum[chunk] + block_scan(k < L ? s.rows[k].points : 0u, part, &total);
    if (k < L) s.rows[k].offset = before;
  }
}

// the tail vertices of the (corner) edges into the member's point array, as far as its cap goes
__global__ void __launch_bounds__(CVH_BLOCK) contour_scatter_kernel(const CvhIoMember *tab, int nmem, int res)
{
  const CvhIoMember *m = section(tab, nmem);
  if (!m->src2) return;   // (no points for this member: wave-uniform)
  const unsigned E = edges_of(m), stride = m->nblk * CVH_BLOCK, w = (unsigned)m->w;
  const unsigned long long cap = (unsigned long long)(unsigned)m->h2 | ((unsigned long long)(unsigned)m->w2 << 32);
  const EdgeSpace s = edge_space(m);
  CVH_GLOBAL int *out = (CVH_GLOBAL int *)m->src2;
  for (unsigned e = (blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x; e < E; e += stride) {
    if (!s.corner[e]) continue;
    const quad a = s.buf[res][e];
    const unsigned loop = ((gwords)(s.buf[res ^ 1] + a.y))[0];
    if (loop >= (unsigned)m->sums[1]) continue;   // (never a row that does not exist)
    const CVH_GLOBAL cvh_contour_loop *row = s.rows + loop;
    const unsigned long long at = row->offset + (a.y == e ? 0u : row->points - a.z);
    if (at >= cap) continue;
    const unsigned id = s.id[e], p = id >> 2;
    int x, y;
    tail_of(id & 3u, (int)(p / w), (int)(p % w), &x, &y);
    out[2 * at] = x;
    out[2 * at + 1] = y;
  }
}

// direction k of an edge: the step from its pixel to the neighbour across it, as (columns, rows)
__device__ __forceinline__ void across(unsigned k, int *dx, int *dy)
{
  *dx = k == 1 ? 1 : (k == 3 ? -1 : 0);
  *dy = k == 2 ? 1 : (k == 0 ? -1 : 0);
}

// the scatter of cvh_contours_subpixel* ("Subpixel contours"; the trace ran with every weight 1): every edge writes, at the place of
// its tail vertex, the point where the zero level crosses the segment between the centres of its pixel and the neighbour across it.
// levels: the mask launches' table of the same members, src the FP64 level set.  FP64 as written: a division, a product with -1, 0 or 1
// and a sum, one rounding each (the build contracts nothing)
__global__ void __launch_bounds__(CVH_BLOCK) contour_scatter_subpixel_kernel(const CvhIoMember *tab, int nmem, int res, const CvhIoMember *levels,
                                                                            int invert)
{
  const CvhIoMember *m = section(tab, nmem);
  if (!m->src2) return;   // (no points for this member: wave-uniform)
  const unsigned E = edges_of(m), stride = m->nblk * CVH_BLOCK, w = (unsigned)m->w;
  const int h = m->h;
  const unsigned long long cap = (unsigned long long)(unsigned)m->h2 | ((unsigned long long)(unsigned)m->w2 << 32);
  const EdgeSpace s = edge_space(m);
  const CVH_GLOBAL double *u = (const CVH_GLOBAL double *)levels[m - tab].src;
  const double sign = invert ? -1.0 : 1.0;
  CVH_GLOBAL point2 *out = (CVH_GLOBAL point2 *)m->src2;
  for (unsigned e = (blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x; e < E; e += stride) {
    const quad a = s.buf[res][e];
    const unsigned loop = ((gwords)(s.buf[res ^ 1] + a.y))[0];
    if (loop >= (unsigned)m->sums[1]) continue;   // (never a row that does not exist)
    const CVH_GLOBAL cvh_contour_loop *row = s.rows + loop;
    const unsigned long long at = row->offset + (a.y == e ? 0u : row->points - a.z);
    if (at >= cap) continue;
    const unsigned id = s.id[e], p = id >> 2;
    const int r = (int)(p / w), c = (int)(p % w);
    int dx, dy;
    across(id & 3u, &dx, &dy);
    const int rq = r + dy, cq = c + dx;
    double t = 0.5;
    if (rq >= 0 && rq < h && cq >= 0 && cq < (int)w) {
      const double va = sign * u[p], vb = sign * u[(size_t)rq * w + (unsigned)cq], d = va - vb;
      if (va > 0.0 && vb <= 0.0 && __builtin_isfinite(d)) t = va / d;
    }
    point2 xy = {((double)c + 0.5) + (double)dx * t, ((double)r + 0.5) + (double)dy * t};
    out[at] = xy;
  }
}

}  // namespace

unsigned cvh_contour_scan_trip() { return 64; }   // counts per trip of contour_scan_kernel's one wave

// workgroups of a member of n pixels with E edges in the edge launches: about four edges a lane, and -- two of the launches go over the
// pixels -- at most sixteen pixels; 2048 at the most, none without edges
unsigned cvh_contour_edge_blocks(size_t edges, size_t n)
{
  if (!edges) return 0;
  const size_t by_edges = (edges + 4 * CVH_BLOCK - 1) / (4 * CVH_BLOCK), by_pixels = (n + 16 * CVH_BLOCK - 1) / (16 * CVH_BLOCK);
  const size_t b = by_edges > by_pixels ? by_edges : by_pixels;
  return (unsigned)(b > 2048 ? 2048 : b);
}

// bytes of a member's per-pixel workspace: mask bytes, edge sets, prefix words (each 256-byte aligned), a count per 256 pixels
size_t cvh_contour_bits_offset(size_t n) { return (n + 255) & ~(size_t)255; }
size_t cvh_contour_prefix_offset(size_t n) { return 2 * cvh_contour_bits_offset(n); }
size_t cvh_contour_counts_offset(size_t n) { return cvh_contour_prefix_offset(n) + ((n * sizeof(unsigned) + 255) & ~(size_t)255); }
size_t cvh_contour_pixel_bytes(size_t n) { return cvh_contour_counts_offset(n) + (size_t)cvh_cc_blocks(n) * sizeof(unsigned); }

// bytes of a member's per-edge workspace with room for cap edges (EdgeSpace): 45 a edge and a little
size_t cvh_contour_edge_bytes(size_t cap)
{
  return 2 * cap * sizeof(quad) + edge_rows(cap) * sizeof(cvh_contour_loop) + cap * sizeof(unsigned) + edge_chunks(cap) * sizeof(unsigned) +
         edge_chunks(edge_rows(cap)) * sizeof(unsigned) + cap;
}
size_t cvh_contour_rows_offset(size_t cap) { return 2 * cap * sizeof(quad); }

#define CT_LAUNCH(KERNEL, GRID, BLOCK, ...) hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(BLOCK), 0, s, tab, nmem, ##__VA_ARGS__)

// the pixel launches: the edge sets of every member's mask and E into its word 0
hipError_t cvh_launch_contours_count(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  CT_LAUNCH(contour_bits_kernel, grid, CVH_BLOCK);
  CT_LAUNCH(contour_scan_kernel, (unsigned)nmem, 64, 0);
  return hipGetLastError();
}

// the edge launches, `rounds` of doubling among them (2^rounds >= the largest E): the rows of every member's loops in its edge
// workspace, the loop and point counts in its words 1 and 2, with any_points the points where a member has an array: lattice points
// (int32 x, y), or with `levels` -- the mask launches' table, the level sets in src; simplify 0 -- the subpixel points (double x, y)
hipError_t cvh_launch_contours_trace(const CvhIoMember *tab, int nmem, unsigned grid, int conn, int simplify, int rounds, bool any_points,
                                     const CvhIoMember *levels, int invert, hipStream_t s)
{
  CT_LAUNCH(contour_prefix_kernel, grid, CVH_BLOCK);
  CT_LAUNCH(contour_link_kernel, grid, CVH_BLOCK, conn, simplify ? 1 : 0);
  for (int r = 0; r < rounds; ++r) CT_LAUNCH(contour_double_kernel, grid, CVH_BLOCK, r & 1);
  const int res = rounds & 1;
  CT_LAUNCH(contour_heads_kernel, grid, CVH_BLOCK, res);
  CT_LAUNCH(contour_scan_kernel, (unsigned)nmem, 64, 1);
  CT_LAUNCH(contour_rows_kernel, grid, CVH_BLOCK, res);
  CT_LAUNCH(contour_sums_kernel, grid, CVH_BLOCK, res);
  CT_LAUNCH(contour_loop_sums_kernel, grid, CVH_BLOCK);
  CT_LAUNCH(contour_scan_kernel, (unsigned)nmem, 64, 2);
  CT_LAUNCH(contour_offsets_kernel, grid, CVH_BLOCK);
  if (any_points && !levels) CT_LAUNCH(contour_scatter_kernel, grid, CVH_BLOCK, res);
  if (any_points && levels) CT_LAUNCH(contour_scatter_subpixel_kernel, grid, CVH_BLOCK, res, levels, invert ? 1 : 0);
  return hipGetLastError();
}
