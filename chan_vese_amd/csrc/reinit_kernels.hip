// reinit_kernels.hip — level-set reinitialisation (cvh_reinit, cvh_reinit_batch; gfx950): the exact signed Euclidean distance to the
// pixel-edge front of the mask ((float)u > 0), in integers until one correctly rounded sqrt per pixel.  Separable transform in three
// launches, each ONE grid over N members of mixed shapes (CvhIoMember, cvh_internal.h; the member table is read through the scalar
// cache); the launches are ordered by their kernel boundaries alone -- no workgroup waits for another.
//   1. reinit_bits_kernel   reads u once.  The plane is cut into bands of 32 rows; a lane owns one column of one band and packs the class
//                           of its 32 pixels into one word (bit r = row r of the band is inside).  Also ORs {an outside pixel exists, an
//                           inside pixel exists} into the member's flag word: a uniform mask makes launches 2 and 3 no-ops.
//   2. reinit_columns_kernel  a lane owns the same column of the same band: the nearest inside / outside row above and below come from
//                           its own word by clz / ctz, and where the band has none from the words of the bands above / below (the FIX-UP:
//                           a scan over at most h / 32 words, coalesced across the lanes' columns).  Writes the two vertical distance fields
//                           g0 (to the nearest outside pixel of the column) and g1 (inside) as one ushort2 per pixel, 0xffff = none:
//                           a finite distance is <= h - 1 <= 65534 for every plane the call accepts (h^2 + w^2 < 2^32).
//   3. reinit_rows_kernel   a workgroup owns a row: g0^2 and g1^2 of the row are staged in LDS (8 bytes per column), then a lane minimises
//                           k^2 + g(j +- k)^2 of the OTHER class outwards from its own column and stops at k^2 >= best -- at most
//                           min(vertical distance, max(j, w - 1 - j)) trips.  u' = +-(sqrt((double)d2) - 0.5).  Rows wider than the LDS
//                           window (8192 columns) read the squares' roots from global memory instead.  A member's first workgroup clears
//                           what a new run clears (as io_checkerboard_kernel).
// No floating-point sum anywhere: the result does not depend on the grid.
#include "cvh_internal.h"

namespace {

#define CVH_GLOBAL __attribute__((address_space(1)))

constexpr unsigned kNone = 0xffffu;          // no pixel of that class in the column
constexpr unsigned kNoneSq = 0xffffffffu;    // its "square": larger than every d2 (< 2^32 - 1)

// the member whose section holds this workgroup (io_kernels.hip's io_member)
__device__ __forceinline__ int reinit_member(const CvhIoMember *tab, int nmem)
{
  int lo = 0, hi = nmem - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// rows of band b that exist, as a bit mask
__device__ __forceinline__ unsigned band_rows(int b, int h)
{
  const int rows = h - b * CVH_REINIT_BAND;
  return rows >= 32 ? 0xffffffffu : ((1u << rows) - 1u);
}

// the workgroups of a member in launches 1 and 2: band-major, 256 columns each
struct ColumnSlot { int band, col; bool live; };
__device__ __forceinline__ ColumnSlot column_slot(const CvhIoMember *m)
{
  const int chunks = (m->w + CVH_BLOCK - 1) / CVH_BLOCK, wg = (int)(blockIdx.x - m->first);
  ColumnSlot s;
  s.band = wg / chunks;
  s.col = (wg % chunks) * CVH_BLOCK + (int)threadIdx.x;
  s.live = s.col < m->w;
  return s;
}

__global__ void __launch_bounds__(CVH_BLOCK) reinit_bits_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned seen[CVH_BLOCK / 64];
  const CvhIoMember *m = tab + reinit_member(tab, nmem);
  const int h = m->h, w = m->w;
  const ColumnSlot s = column_slot(m);
  CVH_GLOBAL const double *u = (CVH_GLOBAL const double *)m->src;
  CVH_GLOBAL unsigned *bits = (CVH_GLOBAL unsigned *)m->plane[0];
  unsigned mine = 0;
  if (s.live) {
    const int r0 = s.band * CVH_REINIT_BAND, rows = h - r0 < CVH_REINIT_BAND ? h - r0 : CVH_REINIT_BAND;
    unsigned word = 0;
    for (int r = 0; r < rows; ++r) word |= (((float)u[(size_t)(r0 + r) * w + s.col] > 0.0f) ? 1u : 0u) << r;   // cvh_get_mask's rule
    bits[(size_t)s.band * w + s.col] = word;
    mine = (word != band_rows(s.band, h) ? 1u : 0u) | (word != 0 ? 2u : 0u);
  }
  // {outside seen, inside seen} of the workgroup; one atomic OR per workgroup, and none once the member's word already holds the bits
  for (int off = 32; off > 0; off >>= 1) mine |= __shfl_down(mine, off, 64);
  if ((threadIdx.x & 63) == 0) seen[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned all = seen[0] | seen[1] | seen[2] | seen[3];
    unsigned *flags = (unsigned *)m->sums;
    if (all & ~__hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(flags, all);
  }
}

__global__ void __launch_bounds__(CVH_BLOCK) reinit_columns_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + reinit_member(tab, nmem);
  if ((*(const unsigned *)m->sums & 3u) != 3u) return;   // uniform mask: nothing to do (wave-uniform)
  const int h = m->h, w = m->w, nbands = (h + CVH_REINIT_BAND - 1) / CVH_REINIT_BAND;
  const ColumnSlot s = column_slot(m);
  if (!s.live) return;
  CVH_GLOBAL const unsigned *bits = (CVH_GLOBAL const unsigned *)m->plane[0];
  CVH_GLOBAL unsigned *g = (CVH_GLOBAL unsigned *)m->plane[1];   // {g0, g1} as two 16-bit halves
  const unsigned valid = band_rows(s.band, h);
  const unsigned word = bits[(size_t)s.band * w + s.col];
  const unsigned cls[2] = {~word & valid, word};   // rows of the band that are outside / inside
  // fix-up: the nearest row of either class above and below the band (-1: none)
  int above[2] = {-1, -1}, below[2] = {-1, -1};
  for (int b = s.band - 1; b >= 0 && (above[0] < 0 || above[1] < 0); --b) {
    const unsigned wd = bits[(size_t)b * w + s.col], c[2] = {~wd, wd};   // (bands above the last one are whole)
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (above[k] < 0 && c[k]) above[k] = b * CVH_REINIT_BAND + 31 - __builtin_clz(c[k]);
  }
  for (int b = s.band + 1; b < nbands && (below[0] < 0 || below[1] < 0); ++b) {
    const unsigned wd = bits[(size_t)b * w + s.col], c[2] = {~wd & band_rows(b, h), wd};
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (below[k] < 0 && c[k]) below[k] = b * CVH_REINIT_BAND + __builtin_ctz(c[k]);
  }
  const int r0 = s.band * CVH_REINIT_BAND, rows = h - r0 < CVH_REINIT_BAND ? h - r0 : CVH_REINIT_BAND;
  for (int r = 0; r < rows; ++r) {
    const int i = r0 + r;
    unsigned d[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned up = cls[k] & (0xffffffffu >> (31 - r)), down = cls[k] >> r;   // rows <= r / rows >= r of the band
      const int ia = up ? r0 + 31 - __builtin_clz(up) : above[k], ib = down ? i + __builtin_ctz(down) : below[k];
      unsigned best = kNone;
      if (ia >= 0) best = (unsigned)(i - ia);
      if (ib >= 0 && (unsigned)(ib - i) < best) best = (unsigned)(ib - i);
      d[k] = best;
    }
    g[(size_t)i * w + s.col] = d[0] | (d[1] << 16);
  }
}

__device__ __forceinline__ unsigned squared(unsigned d) { return d == kNone ? kNoneSq : d * d; }

// LDS: the row's squares live in LDS, [0, w) towards outside pixels and [w, 2w) towards inside pixels; else they are taken from global memory
template <bool LDS>
__device__ __forceinline__ unsigned other_sq(const unsigned *sq, CVH_GLOBAL const unsigned *grow, int w, int j, bool inside)
{
  if (LDS) return sq[(inside ? 0 : w) + j];
  const unsigned v = grow[j];
  return squared(inside ? (v & 0xffffu) : (v >> 16));
}

template <bool LDS>
__device__ __forceinline__ void reinit_row(const unsigned *sq, CVH_GLOBAL const unsigned *grow, CVH_GLOBAL double *out, int w)
{
  for (int j = (int)threadIdx.x; j < w; j += CVH_BLOCK) {
    const bool inside = LDS ? sq[w + j] == 0 : (grow[j] >> 16) == 0;   // g1 == 0: the pixel itself is inside
    unsigned best = other_sq<LDS>(sq, grow, w, j, inside);
    const unsigned kmax = (unsigned)(j > w - 1 - j ? j : w - 1 - j);
    for (unsigned k = 1; k <= kmax; ++k) {
      const unsigned k2 = k * k;   // (k < w <= 65535)
      if (k2 >= best) break;
      if ((unsigned)j >= k) {
        const unsigned c = k2 + other_sq<LDS>(sq, grow, w, j - (int)k, inside);   // wraps below k2 exactly when the column has none
        if (c >= k2 && c < best) best = c;
      }
      if ((unsigned)j + k < (unsigned)w) {
        const unsigned c = k2 + other_sq<LDS>(sq, grow, w, j + (int)k, inside);
        if (c >= k2 && c < best) best = c;
      }
    }
    const double d = sqrt((double)best) - 0.5;   // IEEE sqrt, one subtraction (the unit is built without FMA contraction)
    out[j] = inside ? d : -d;
  }
}

__global__ void __launch_bounds__(CVH_BLOCK) reinit_rows_kernel(const CvhIoMember *tab, int nmem)
{
  extern __shared__ unsigned sq[];
  const CvhIoMember *m = tab + reinit_member(tab, nmem);
  if ((*(const unsigned *)m->sums & 3u) != 3u) return;   // uniform mask: the level set stays as it is
  const int h = m->h, w = m->w, wg = (int)(blockIdx.x - m->first), nblk = (int)m->nblk;
  CVH_GLOBAL const unsigned *g = (CVH_GLOBAL const unsigned *)m->plane[1];
  CVH_GLOBAL double *out = (CVH_GLOBAL double *)m->dst;
  if (wg == 0) {   // the device's share of a new run (reset_run_impl)
    if (threadIdx.x < 4) ((CVH_GLOBAL int *)m->state_zero)[threadIdx.x] = 0;
    if (threadIdx.x < 64) ((CVH_GLOBAL long long *)m->chain_zero)[threadIdx.x] = 0;
  }
  const bool lds = w <= CVH_REINIT_LDS_COLS;   // (wave-uniform: a member's width)
  for (int i = wg; i < h; i += nblk) {
    CVH_GLOBAL const unsigned *grow = g + (size_t)i * w;
    if (lds) {
      __syncthreads();   // the previous row's squares have been read
      for (int j = (int)threadIdx.x; j < w; j += CVH_BLOCK) {
        const unsigned v = grow[j];
        sq[j] = squared(v & 0xffffu);
        sq[w + j] = squared(v >> 16);
      }
      __syncthreads();
      reinit_row<true>(sq, grow, out + (size_t)i * w, w);
    } else {
      reinit_row<false>(sq, grow, out + (size_t)i * w, w);
    }
  }
}

}  // namespace

unsigned cvh_reinit_column_blocks(int h, int w)
{
  return (unsigned)(((h + CVH_REINIT_BAND - 1) / CVH_REINIT_BAND) * ((w + CVH_BLOCK - 1) / CVH_BLOCK));
}

unsigned cvh_reinit_row_blocks(int h) { return (unsigned)(h < 8192 ? h : 8192); }

// bytes of a member's workspace: the class words of every band, then the two distance fields (16-byte aligned)
size_t cvh_reinit_bits_bytes(int h, int w)
{
  const size_t b = (size_t)((h + CVH_REINIT_BAND - 1) / CVH_REINIT_BAND) * (size_t)w * sizeof(unsigned);
  return (b + 255) & ~(size_t)255;
}
size_t cvh_reinit_workspace_bytes(int h, int w) { return cvh_reinit_bits_bytes(h, w) + (size_t)h * (size_t)w * sizeof(unsigned); }

// the three launches of one reinitialisation: cols / rows are the member tables of launches 1 + 2 and of launch 3 (same members, their own
// first / nblk), max_w the widest member (sizes the LDS window of launch 3)
hipError_t cvh_launch_reinit(const CvhIoMember *cols, unsigned col_grid, const CvhIoMember *rows, unsigned row_grid, int nmem, int max_w,
                             hipStream_t s)
{
  const int lds_cols = max_w <= CVH_REINIT_LDS_COLS ? max_w : CVH_REINIT_LDS_COLS;
  hipLaunchKernelGGL(reinit_bits_kernel, dim3(col_grid), dim3(CVH_BLOCK), 0, s, cols, nmem);
  hipLaunchKernelGGL(reinit_columns_kernel, dim3(col_grid), dim3(CVH_BLOCK), 0, s, cols, nmem);
  hipLaunchKernelGGL(reinit_rows_kernel, dim3(row_grid), dim3(CVH_BLOCK), (size_t)lds_cols * 2 * sizeof(unsigned), s, rows, nmem);
  return hipGetLastError();
}
