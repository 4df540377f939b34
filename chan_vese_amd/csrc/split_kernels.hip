// split_kernels.hip — object split (cvh_split*, cvh_split_levelset*; include/chanvese_hip.h "Object split"; gfx950): the launches the
// family adds to the erosion passes of morph_kernels.hip and the labelling launches of components_kernels.hip, which it reuses through
// their host entry points.  Everything is integers and every launch is ONE grid over N members of mixed shapes (CvhIoMember); the
// launches are ordered by their kernel boundaries alone -- no workgroup waits for or polls another.
//   split_flag_kernel     a pixel of the eroded set E raises the flag of its F0 component: a vector atomic OR on the statistics word of the
//                         component's root (the flattened forest of F0 the labelling launches left).
//   split_marker_kernel   M as a byte plane: a pixel of F0 that is in E, or whose component has no flag.
//   split_keys_kernel     behind the labelling of M: key(p) = m(p) on M (d = 0), kUnreached on F0 \ M, 0 outside F0 -- into the key plane,
//                         which is the member's plane rounded up to whole tiles (the padding is outside F0).
//   split_sweep_kernel    THE GROWTH.  A key is 64 bits, (d << 32) | L: d < h w < 2^31 and L <= K <= 2^30 both fit, so the family's cap is
//                         the labelling's h w < 2^31 and nothing narrower.  A workgroup owns a tile of CVH_SPLIT_TILE_ROWS x
//                         CVH_SPLIT_TILE_COLS keys plus a one-pixel halo, loads them into LDS (the interior in 16-byte pieces, which
//                         no other workgroup writes; the halo key by key with relaxed atomic loads, because the neighbour tile's
//                         workgroup may be storing it), relaxes key(p) = min(key(p), min_q key(q) + (1 << 32)) over the conn-neighbours
//                         q in F0 until the tile is stable, stores the keys that fell (relaxed atomic 64-bit stores: a racing halo load
//                         sees the old key or the new one, both upper bounds of the fixpoint) and adds their number to the member's
//                         counter of this sweep with one vector atomic add.  A member whose counter of the sweep before is zero is at
//                         its fixpoint: its workgroups return at once.
//   split_emit_kernel     the cut and the outputs in one launch: L is a key's low word; cut(p) iff some 8-neighbour has a larger label;
//                         int32 labels at any 4-byte aligned address, or the level set (inside on F0 \ cut, outside elsewhere), four
//                         pixels per lane written in 16-byte pieces.
//   split_table_*         a table's rows from L, as cc_table_*: `first` from the numbered roots of M's forest, area and box per horizontal
//                         run inside a wave.
#include "cc_device.h"
#include "io_device.h"

namespace {

typedef unsigned long long key_t;
typedef CVH_GLOBAL key_t *gkeys;
typedef CVH_GLOBAL unsigned *gwords;
typedef key_t v2k __attribute__((ext_vector_type(2)));

constexpr key_t kOne = 1ull << 32;                   // one step of d
constexpr key_t kUnreached = 0x7fffffffull << 32;    // a pixel of F0 no marker has reached yet (kUnreached + kOne does not wrap)
constexpr unsigned kNone = kCcNone, kNumbered = kCcNumbered;   // (cc_device.h: the marks of a parent word)
constexpr int TR = CVH_SPLIT_TILE_ROWS, TC = CVH_SPLIT_TILE_COLS, LP = TC + 2;   // LDS pitch in keys
static_assert(CVH_BLOCK == 256 && TC == 64 && TR == 32, "a wave owns 8 rows of the tile, a lane one column");

struct Pixel { const CvhIoMember *m; unsigned p; bool live; };
__device__ __forceinline__ Pixel split_pixel(const CvhIoMember *tab, int nmem)
{
  Pixel x;
  x.m = tab + io_member(tab, nmem);
  x.p = (blockIdx.x - x.m->first) * CVH_BLOCK + threadIdx.x;   // (h w < 2^31)
  x.live = x.p < (unsigned)x.m->n;
  return x;
}

// the root of a pixel of the class in a flattened forest, numbered or not
__device__ __forceinline__ unsigned root_of(gwords parent, unsigned p)
{
  const unsigned v = parent[p];
  return (v & kNumbered) ? p : v;
}

__device__ __forceinline__ bool eroded(const CvhIoMember *m, unsigned p)
{
  const unsigned w = (unsigned)m->w, i = p / w, j = p - i * w;
  return (((CVH_GLOBAL const unsigned *)m->src2)[(size_t)(i >> 5) * w + j] >> (i & 31)) & 1u;
}

// table: src the bytes of F0, src2 the band words of E, plane[0] / plane[1] the parent and statistics words of F0's forest
__global__ void __launch_bounds__(CVH_BLOCK) split_flag_kernel(const CvhIoMember *tab, int nmem)
{
  const Pixel x = split_pixel(tab, nmem);
  if (!x.live || !((gbytes_in)x.m->src)[x.p] || !eroded(x.m, x.p)) return;
  const gwords stat = (gwords)x.m->plane[1];
  const unsigned root = root_of((gwords)x.m->plane[0], x.p);
  if (!__hip_atomic_load(stat + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    __hip_atomic_fetch_or(stat + root, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the same table; dst the bytes of M
__global__ void __launch_bounds__(CVH_BLOCK) split_marker_kernel(const CvhIoMember *tab, int nmem)
{
  const Pixel x = split_pixel(tab, nmem);
  if (!x.live) return;
  bool in = ((gbytes_in)x.m->src)[x.p] != 0;
  if (in && !eroded(x.m, x.p)) in = ((gwords)x.m->plane[1])[root_of((gwords)x.m->plane[0], x.p)] == 0;
  ((gbytes_out)x.m->dst)[x.p] = in ? 1 : 0;
}

// table: src the parent words of M's numbered forest, src2 the bytes of F0, plane[0] the key plane, w2 its pitch in keys
__global__ void __launch_bounds__(CVH_BLOCK) split_keys_kernel(const CvhIoMember *tab, int nmem)
{
  const Pixel x = split_pixel(tab, nmem);
  if (!x.live) return;
  CVH_GLOBAL const unsigned *parent = (CVH_GLOBAL const unsigned *)x.m->src;
  const unsigned v = parent[x.p], w = (unsigned)x.m->w, i = x.p / w, j = x.p - i * w;
  key_t k = ((gbytes_in)x.m->src2)[x.p] ? kUnreached : 0;
  if (v != kNone) k = ((v & kNumbered) ? v : parent[v]) & ~kNumbered;
  ((gkeys)x.m->plane[0])[(size_t)i * (unsigned)x.m->w2 + j] = k;
}

__device__ __forceinline__ key_t step_from(key_t q) { return q ? q + kOne : ~0ull; }   // (0: not a pixel of F0)

// table: plane[0] the key plane, h2 / w2 its rows and pitch (whole tiles), interleaved the tiles per row, sums the member's counter of
// slot 0 (32-bit words, `stride` words between the slots); the sweep reads slot `slot` and adds to slot + 1
__global__ void __launch_bounds__(CVH_BLOCK) split_sweep_kernel(const CvhIoMember *tab, int nmem, int conn, int slot, int stride)
{
  __shared__ key_t t[(TR + 2) * LP];
  __shared__ unsigned fell[CVH_BLOCK / 64];
  const CvhIoMember *m = tab + io_member(tab, nmem);
  CVH_GLOBAL unsigned *cnt = (CVH_GLOBAL unsigned *)m->sums + (size_t)slot * stride;
  if (!__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;   // (wave-uniform: the member's)
  const int wg = (int)(blockIdx.x - m->first), tx = wg % m->interleaved, ty = wg / m->interleaved;
  const int Hp = m->h2, Wp = m->w2, r0 = ty * TR, c0 = tx * TC;
  const gkeys keys = (gkeys)m->plane[0];
  // the interior: a lane takes two neighbouring keys, 32 lanes a row (Wp and c0 are multiples of 64: 16-byte aligned)
  for (int q = threadIdx.x; q < TR * TC / 2; q += CVH_BLOCK) {
    const int r = q / (TC / 2), c = 2 * (q % (TC / 2));
    const v2k v = *(CVH_GLOBAL const v2k *)(keys + (size_t)(r0 + r) * Wp + c0 + c);
    t[(r + 1) * LP + c + 1] = v.x;
    t[(r + 1) * LP + c + 2] = v.y;
  }
  // the halo: rows -1 and TR with their corners, then columns -1 and TC; outside the key plane nothing is of F0
  for (int q = threadIdx.x; q < 2 * LP + 2 * TR; q += CVH_BLOCK) {
    int r, c;
    if (q < 2 * LP) { r = q < LP ? -1 : TR; c = (q < LP ? q : q - LP) - 1; }
    else { const int e = q - 2 * LP; r = e >> 1; c = (e & 1) ? TC : -1; }
    const int gr = r0 + r, gc = c0 + c;
    key_t v = 0;
    if (gr >= 0 && gr < Hp && gc >= 0 && gc < Wp) v = __hip_atomic_load(keys + (size_t)gr * Wp + gc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t[(r + 1) * LP + c + 1] = v;
  }
  __syncthreads();
  // a lane owns column `col` of the 8 rows of its wave: reads are rounds apart from writes (a barrier each), so no key is read half written
  const int col = (int)(threadIdx.x & 63u) + 1, row = (int)(threadIdx.x >> 6) * 8 + 1;
  key_t k[8], was[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = was[j] = t[(row + j) * LP + col];
  for (;;) {
    bool moved = false;
    key_t up = t[(row - 1) * LP + col];
#pragma unroll
    for (int j = 0; j < 8; ++j) {   // downwards: the key just lowered above is this pixel's neighbour already
      const key_t *c = t + (row + j) * LP + col;
      key_t best = step_from(up);
      best = min(best, step_from(c[-1]));
      best = min(best, step_from(c[1]));
      if (j == 7) best = min(best, step_from(c[LP]));
      if (conn == 8) {
        best = min(best, min(step_from(c[-LP - 1]), step_from(c[-LP + 1])));
        best = min(best, min(step_from(c[LP - 1]), step_from(c[LP + 1])));
      }
      if (k[j] && best < k[j]) { k[j] = best; moved = true; }
      up = k[j];
    }
#pragma unroll
    for (int j = 6; j >= 0; --j) {   // and upwards
      const key_t best = step_from(k[j + 1]);
      if (k[j] && best < k[j]) { k[j] = best; moved = true; }
    }
    if (!__syncthreads_or(moved ? 1 : 0)) break;   // (every read of the round is done)
#pragma unroll
    for (int j = 0; j < 8; ++j) t[(row + j) * LP + col] = k[j];
    __syncthreads();
  }
  unsigned mine = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (k[j] == was[j]) continue;
    __hip_atomic_store(keys + (size_t)(r0 + row - 1 + j) * Wp + c0 + col - 1, k[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ++mine;
  }
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
  if ((threadIdx.x & 63u) == 0) fell[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned all = fell[0] + fell[1] + fell[2] + fell[3];
    if (all) __hip_atomic_fetch_add(cnt + stride, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// L of pixel (i, j); 0 outside the plane
__device__ __forceinline__ unsigned label_at(gkeys keys, int Wp, int h, int w, int i, int j)
{
  if (i < 0 || i >= h || j < 0 || j >= w) return 0;
  return (unsigned)keys[(size_t)i * Wp + j];
}

// table: plane[0] the key plane, w2 its pitch, dst the int32 labels (may be null) or the level set with state_zero / chain_zero as the
// checkerboard's; sections of cvh_split_emit_blocks(n) workgroups, four pixels per lane
template <bool TO_LEVELSET>
__global__ void __launch_bounds__(CVH_BLOCK) split_emit_kernel(const CvhIoMember *tab, const CvhMorphPar *par, int nmem)
{
  const int mi = io_member(tab, nmem);
  const CvhIoMember *m = tab + mi;
  const int wg = (int)(blockIdx.x - m->first), h = m->h, w = m->w, Wp = m->w2;
  if (TO_LEVELSET && wg == 0) {   // the device's share of a new run (reset_run_impl)
    if (threadIdx.x < 4) ((CVH_GLOBAL int *)m->state_zero)[threadIdx.x] = 0;
    if (threadIdx.x < 64) ((CVH_GLOBAL long long *)m->chain_zero)[threadIdx.x] = 0;
  }
  if (!m->dst) return;   // (a member without a label plane: wave-uniform)
  const size_t n = m->n, p0 = 4 * ((size_t)wg * CVH_BLOCK + threadIdx.x);
  if (p0 >= n) return;
  const gkeys keys = (gkeys)m->plane[0];
  unsigned L[4] = {0, 0, 0, 0};
  bool cut[4] = {false, false, false, false};
  int i = (int)(p0 / (size_t)w), j = (int)(p0 - (size_t)i * w);
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    if (p0 + b < n) {
      const unsigned l = label_at(keys, Wp, h, w, i, j);
      L[b] = l;
      if (TO_LEVELSET && l) {
        unsigned top = 0;
        for (int di = -1; di <= 1; ++di)
          for (int dj = -1; dj <= 1; ++dj) top = max(top, label_at(keys, Wp, h, w, i + di, j + dj));
        cut[b] = top > l;
      }
      if (++j == w) { j = 0; ++i; }
    }
  }
  if (TO_LEVELSET) {
    CVH_GLOBAL double *u = (CVH_GLOBAL double *)m->dst;
    const double inside = par[mi].inside, outside = par[mi].outside;
    double o[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) o[b] = L[b] && !cut[b] ? inside : outside;
    if (p0 + 4 <= n) {
      const v2d lo = {o[0], o[1]}, hi = {o[2], o[3]};
      ((CVH_GLOBAL v2d *)(u + p0))[0] = lo;
      ((CVH_GLOBAL v2d *)(u + p0))[1] = hi;
    } else {
      for (int b = 0; p0 + b < n; ++b) u[p0 + b] = o[b];
    }
  } else {
    CVH_GLOBAL int *out = (CVH_GLOBAL int *)m->dst;
    if (p0 + 4 <= n) store16_any((gbytes_out)(out + p0), make_uint4(L[0], L[1], L[2], L[3]));
    else for (int b = 0; p0 + b < n; ++b) out[p0 + b] = (int)L[b];
  }
}

// table rows (the member's dst): src the parent words of M's numbered forest -- a root writes `first` and the neutral elements
__global__ void __launch_bounds__(CVH_BLOCK) split_table_init_kernel(const CvhIoMember *tab, int nmem)
{
  const Pixel x = split_pixel(tab, nmem);
  if (!x.live) return;
  const unsigned v = ((CVH_GLOBAL const unsigned *)x.m->src)[x.p];
  if (v == kNone || !(v & kNumbered)) return;
  CVH_GLOBAL cvh_component *row = (CVH_GLOBAL cvh_component *)x.m->dst + ((v & ~kNumbered) - 1u);
  cc_row_init(row, x.p);
}

// area and box of { L = k }: one set of atomics per horizontal run of a label inside a wave (cc_device.h, as cc_table_stats_kernel)
__global__ void __launch_bounds__(CVH_BLOCK) split_table_stats_kernel(const CvhIoMember *tab, int nmem)
{
  const Pixel x = split_pixel(tab, nmem);
  const unsigned w = (unsigned)x.m->w, i = x.live ? x.p / w : 0u, c = x.live ? x.p - i * w : 0u;
  const unsigned k = x.live ? (unsigned)((gkeys)x.m->plane[0])[(size_t)i * (unsigned)x.m->w2 + c] : 0u;
  const unsigned len = cc_run_length(k ? k : kNone, c == 0);
  if (!len) return;
  cc_row_add_run((CVH_GLOBAL cvh_component *)x.m->dst + (k - 1u), len, (int)i, (int)c);
}

}  // namespace

unsigned cvh_split_emit_blocks(size_t n) { return (unsigned)((n + 4 * CVH_BLOCK - 1) / (4 * CVH_BLOCK)); }

#define SPLIT_LAUNCH(KERNEL, GRID, ...) hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(CVH_BLOCK), 0, s, ##__VA_ARGS__)

hipError_t cvh_launch_split_markers(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  SPLIT_LAUNCH(split_flag_kernel, grid, tab, nmem);
  SPLIT_LAUNCH(split_marker_kernel, grid, tab, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_split_keys(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  SPLIT_LAUNCH(split_keys_kernel, grid, tab, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_split_sweeps(const CvhIoMember *tiles, int nmem, unsigned tile_grid, int conn, int sweeps, hipStream_t s)
{
  for (int j = 0; j < sweeps; ++j) SPLIT_LAUNCH(split_sweep_kernel, tile_grid, tiles, nmem, conn, j, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_split_emit(const CvhIoMember *tab, const CvhMorphPar *par, int nmem, unsigned grid, bool to_levelset, hipStream_t s)
{
  if (to_levelset) SPLIT_LAUNCH(split_emit_kernel<true>, grid, tab, par, nmem);
  else SPLIT_LAUNCH(split_emit_kernel<false>, grid, tab, par, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_split_table(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  SPLIT_LAUNCH(split_table_init_kernel, grid, tab, nmem);
  SPLIT_LAUNCH(split_table_stats_kernel, grid, tab, nmem);
  return hipGetLastError();
}
