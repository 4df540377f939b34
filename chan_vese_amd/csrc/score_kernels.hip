// score_kernels.hip — mask scores (cvh_score_mask*, include/chanvese_hip.h "Mask scores"; gfx950): the mask M of the level set against a
// ground-truth plane T, in integers throughout -- the four overlap counts, the sizes of the two 4-neighbour surfaces, and per surface the
// maximum, the 16.16 sum and the count-within-tolerance of the exact squared distance to the other surface.  The work is the
// reinitialisation's separable transform (reinit_kernels.hip) with two changes: the two sets are surfaces, not classes, and only surface
// pixels search.  Four launches, each ONE grid over N members of mixed shapes (CvhIoMember, cvh_internal.h), ordered by their kernel
// boundaries alone -- no workgroup waits for another:
//   1. score_class_kernel    reads u and the truth bytes once.  A lane owns one column of a band of 32 rows and packs M and T of its 32
//                            pixels into two words; tp / fp / fn / tn are popcounts, reduced across the wave and the workgroup.
//   2. score_surface_kernel  the surface words from the class words: left / right from the neighbouring columns' words, up / down by
//                            shifts and from the adjacent bands' words at bits 31 / 0; what lies outside the plane is outside the set.
//                            Counts surf_m / surf_t.  (A launch of its own: launch 3's fix-up reads the surface words of OTHER bands,
//                            which only a kernel boundary orders behind their writers.)
//   3. score_columns_kernel  reinit_columns_kernel on the two surface planes: per pixel the vertical distance to the nearest pixel of
//                            surf(T) and of surf(M) in its column, one unsigned per pixel {low half: T, high half: M}, 0xffff = none.
//   4. score_rows_kernel     a workgroup owns a row.  The row's distance words are staged in LDS and its surface columns are COMPACTED
//                            into two lists (ballot + popcount prefix per wave, one LDS add per wave for the wave's base), so that
//                            the lanes each take a surface pixel instead of a column: only O(perimeter) pixels of a row search.  A
//                            pixel of surf(M) minimises k^2 + g_T(j +- k)^2 outwards from its column and stops at k^2 >= best; a
//                            pixel of surf(T) does the same against g_M.  Rows wider than the LDS window (8192 columns) take a lane
//                            per column and read the words from global memory.
// A member with an empty surface (the result row's surf_m or surf_t is 0 behind launch 2) returns at once from launches 3 and 4.
// Every sum is an integer and every combination a 64-bit add or a 32-bit max: one vector atomic per workgroup and field behind a
// wave and workgroup reduction; the result does not depend on the grid, the arrival order or the batch.
#include "cvh_internal.h"

namespace {

#define CVH_GLOBAL __attribute__((address_space(1)))

constexpr unsigned kNone = 0xffffu;          // no pixel of that surface in the column
constexpr unsigned kNoneSq = 0xffffffffu;    // its "square": larger than every d2 (< 2^32 - 1)
constexpr int kWaves = CVH_BLOCK / 64;

// the member whose section holds this workgroup (io_kernels.hip's io_member)
__device__ __forceinline__ int score_member(const CvhIoMember *tab, int nmem)
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

// the workgroups of a member in launches 1 - 3: band-major, 256 columns each
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

// plane k of the member's band words: 0 class of M, 1 class of T, 2 surf(M), 3 surf(T)
__device__ __forceinline__ CVH_GLOBAL unsigned *words_plane(const CvhIoMember *m, int k)
{
  return (CVH_GLOBAL unsigned *)(m->plane[0] + (size_t)k * cvh_score_words_bytes(m->h, m->w));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v)
{
  for (int off = 32; off > 0; off >>= 1) { const unsigned o = __shfl_down(v, off, 64); v = o > v ? o : v; }
  return v;
}

// N per-lane counts become N 64-bit adds of the workgroup into row[first ..]: lane 0 of every wave parks the wave's sums in LDS, thread k
// adds column k.  Zero sums are not sent.  (All threads of the workgroup arrive here.)
template <int N>
__device__ __forceinline__ void workgroup_add(unsigned long long (*part)[kWaves], const unsigned long long (&mine)[N], unsigned long long *row, int first)
{
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const unsigned long long s = wave_sum(mine[k]);
    if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    unsigned long long s = 0;
    for (int v = 0; v < kWaves; ++v) s += part[threadIdx.x][v];
    if (s) atomicAdd(row + first + threadIdx.x, s);
  }
}

__global__ void __launch_bounds__(CVH_BLOCK) score_class_kernel(const CvhIoMember *tab, int nmem, int invert)
{
  __shared__ unsigned long long part[4][kWaves];
  const CvhIoMember *m = tab + score_member(tab, nmem);
  const int h = m->h, w = m->w;
  const ColumnSlot s = column_slot(m);
  CVH_GLOBAL const double *u = (CVH_GLOBAL const double *)m->src;
  CVH_GLOBAL const unsigned char *t = (CVH_GLOBAL const unsigned char *)m->src2;
  unsigned long long mine[4] = {0, 0, 0, 0};
  if (s.live) {
    const int r0 = s.band * CVH_REINIT_BAND, rows = h - r0 < CVH_REINIT_BAND ? h - r0 : CVH_REINIT_BAND;
    unsigned wm = 0, wt = 0;
    for (int r = 0; r < rows; ++r) {
      const size_t p = (size_t)(r0 + r) * w + s.col;
      wm |= ((((float)u[p] > 0.0f) != (invert != 0)) ? 1u : 0u) << r;   // cvh_get_mask's rule
      wt |= (t[p] != 0 ? 1u : 0u) << r;
    }
    words_plane(m, 0)[(size_t)s.band * w + s.col] = wm;
    words_plane(m, 1)[(size_t)s.band * w + s.col] = wt;
    const unsigned valid = band_rows(s.band, h);
    mine[CVH_SCORE_TP] = (unsigned)__builtin_popcount(wm & wt);
    mine[CVH_SCORE_FP] = (unsigned)__builtin_popcount(wm & ~wt);
    mine[CVH_SCORE_FN] = (unsigned)__builtin_popcount(~wm & wt);
    mine[CVH_SCORE_TN] = (unsigned)__builtin_popcount(~wm & ~wt & valid);
  }
  workgroup_add<4>(part, mine, m->sums, CVH_SCORE_TP);
}

// the pixels of the band's word `mid` with a 4-neighbour outside the set
__device__ __forceinline__ unsigned surface_word(CVH_GLOBAL const unsigned *cls, int band, int nbands, int col, int w)
{
  const size_t at = (size_t)band * w + col;
  const unsigned mid = cls[at];
  if (!mid) return 0;
  const unsigned left = col > 0 ? cls[at - 1] : 0u, right = col + 1 < w ? cls[at + 1] : 0u;
  const unsigned above = band > 0 ? cls[at - (size_t)w] >> 31 : 0u;                  // row 31 of the band above
  const unsigned below = band + 1 < nbands ? (cls[at + (size_t)w] & 1u) << 31 : 0u;    // row 0 of the band below (this band is whole then)
  const unsigned up = (mid << 1) | above, down = (mid >> 1) | below;   // (no bit of `mid` lies past the plane's last row)
  return mid & ~(left & right & up & down);
}

__global__ void __launch_bounds__(CVH_BLOCK) score_surface_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned long long part[2][kWaves];
  const CvhIoMember *m = tab + score_member(tab, nmem);
  const int h = m->h, w = m->w, nbands = (h + CVH_REINIT_BAND - 1) / CVH_REINIT_BAND;
  const ColumnSlot s = column_slot(m);
  unsigned long long mine[2] = {0, 0};
  if (s.live) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned sf = surface_word(words_plane(m, k), s.band, nbands, s.col, w);
      words_plane(m, 2 + k)[(size_t)s.band * w + s.col] = sf;
      mine[k] = (unsigned)__builtin_popcount(sf);
    }
  }
  workgroup_add<2>(part, mine, m->sums, CVH_SCORE_SURF_M);
}

__device__ __forceinline__ bool surfaces_exist(const CvhIoMember *m)
{
  return m->sums[CVH_SCORE_SURF_M] != 0 && m->sums[CVH_SCORE_SURF_T] != 0;   // (written by launch 2: a kernel boundary ago)
}

__global__ void __launch_bounds__(CVH_BLOCK) score_columns_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + score_member(tab, nmem);
  if (!surfaces_exist(m)) return;   // an empty surface: no distance is defined (wave-uniform)
  const int h = m->h, w = m->w, nbands = (h + CVH_REINIT_BAND - 1) / CVH_REINIT_BAND;
  const ColumnSlot s = column_slot(m);
  if (!s.live) return;
  CVH_GLOBAL const unsigned *sf[2] = {words_plane(m, 3), words_plane(m, 2)};   // [0] surf(T), [1] surf(M): the halves of a distance word
  CVH_GLOBAL unsigned *g = (CVH_GLOBAL unsigned *)m->plane[1];
  const unsigned cls[2] = {sf[0][(size_t)s.band * w + s.col], sf[1][(size_t)s.band * w + s.col]};
  // fix-up: the nearest row of either surface above and below the band (-1: none)
  int above[2] = {-1, -1}, below[2] = {-1, -1};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    for (int b = s.band - 1; b >= 0 && above[k] < 0; --b) {
      const unsigned wd = sf[k][(size_t)b * w + s.col];
      if (wd) above[k] = b * CVH_REINIT_BAND + 31 - __builtin_clz(wd);
    }
    for (int b = s.band + 1; b < nbands && below[k] < 0; ++b) {
      const unsigned wd = sf[k][(size_t)b * w + s.col];
      if (wd) below[k] = b * CVH_REINIT_BAND + __builtin_ctz(wd);
    }
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

// the squared distance from column j of the row, a pixel of one surface, to the other surface: gw[.] the row's distance words,
// half = 0 towards surf(T) (the pixel is of surf(M)), 16 towards surf(M)
template <class Words>
__device__ __forceinline__ unsigned nearest_sq(Words gw, int w, int j, int half)
{
  unsigned best = squared((gw[j] >> half) & 0xffffu);
  const unsigned kmax = (unsigned)(j > w - 1 - j ? j : w - 1 - j);
  for (unsigned k = 1; k <= kmax; ++k) {
    const unsigned k2 = k * k;   // (k < w <= 65535)
    if (k2 >= best) break;
    if ((unsigned)j >= k) {
      const unsigned c = k2 + squared((gw[j - (int)k] >> half) & 0xffffu);   // wraps below k2 exactly when the column has none
      if (c >= k2 && c < best) best = c;
    }
    if ((unsigned)j + k < (unsigned)w) {
      const unsigned c = k2 + squared((gw[j + (int)k] >> half) & 0xffffu);
      if (c >= k2 && c < best) best = c;
    }
  }
  return best;
}

// a surface pixel's d2 joins its surface's maximum, count-within and 16.16 sum
__device__ __forceinline__ void book(unsigned &hd2, unsigned long long &within, unsigned long long &dist, unsigned d2, unsigned tol2)
{
  hd2 = d2 > hd2 ? d2 : hd2;
  within += d2 <= tol2 ? 1u : 0u;
  // q16: an IEEE sqrt, an exact multiply by 2^16, a round-half-even to an integer of at most 2^32 (the unit is built without FMA contraction)
  dist += (unsigned long long)rint(sqrt((double)d2) * 65536.0);
}

__global__ void __launch_bounds__(CVH_BLOCK) score_rows_kernel(const CvhIoMember *tab, int nmem, unsigned tol2)
{
  extern __shared__ unsigned lds[];   // [w distance words][w columns of surf(M)][w columns of surf(T)] (16-bit columns): 8 bytes per column
  __shared__ unsigned count[2];
  __shared__ unsigned long long part[4][kWaves];
  __shared__ unsigned top[2][kWaves];
  const CvhIoMember *m = tab + score_member(tab, nmem);
  if (!surfaces_exist(m)) return;   // (wave-uniform, and workgroup-uniform: no barrier is left waiting)
  const int h = m->h, w = m->w, wg = (int)(blockIdx.x - m->first), nblk = (int)m->nblk;
  CVH_GLOBAL const unsigned *g = (CVH_GLOBAL const unsigned *)m->plane[1];
  const int lane = (int)(threadIdx.x & 63);
  unsigned hd_m = 0, hd_t = 0;   // what this lane has found so far, per surface
  unsigned long long in_m = 0, in_t = 0, sum_m = 0, sum_t = 0;
  if (w <= CVH_REINIT_LDS_COLS) {   // (wave-uniform: a member's width)
    unsigned *gw = lds;
    unsigned short *list[2] = {(unsigned short *)(lds + w), (unsigned short *)(lds + w) + w};
    for (int i = wg; i < h; i += nblk) {
      CVH_GLOBAL const unsigned *grow = g + (size_t)i * w;
      __syncthreads();   // the previous row's words and lists have been read
      if (threadIdx.x < 2) count[threadIdx.x] = 0;
      __syncthreads();
      for (int j0 = 0; j0 < w; j0 += CVH_BLOCK) {   // (every lane makes every trip: the ballots are of whole waves)
        const int j = j0 + (int)threadIdx.x;
        const unsigned v = j < w ? grow[j] : 0xffffffffu;
        if (j < w) gw[j] = v;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const bool on = (k ? (v & 0xffffu) : (v >> 16)) == 0;   // the pixel's own distance to its surface is 0
          const unsigned long long vote = __ballot(on);
          unsigned base = 0;
          if (lane == 0 && vote) base = atomicAdd(&count[k], (unsigned)__builtin_popcountll(vote));   // (LDS)
          base = __shfl(base, 0, 64);
          if (on) list[k][base + (unsigned)__builtin_popcountll(vote & ((1ull << lane) - 1ull))] = (unsigned short)j;
        }
      }
      __syncthreads();
      const unsigned n0 = count[0], total = n0 + count[1];
      for (unsigned q = threadIdx.x; q < total; q += CVH_BLOCK) {
        if (q < n0) book(hd_m, in_m, sum_m, nearest_sq(gw, w, (int)list[0][q], 0), tol2);
        else book(hd_t, in_t, sum_t, nearest_sq(gw, w, (int)list[1][q - n0], 16), tol2);
      }
    }
  } else {
    for (int i = wg; i < h; i += nblk) {
      CVH_GLOBAL const unsigned *grow = g + (size_t)i * w;
      for (int j = (int)threadIdx.x; j < w; j += CVH_BLOCK) {
        const unsigned v = grow[j];
        if ((v >> 16) == 0) book(hd_m, in_m, sum_m, nearest_sq(grow, w, j, 0), tol2);
        if ((v & 0xffffu) == 0) book(hd_t, in_t, sum_t, nearest_sq(grow, w, j, 16), tol2);
      }
    }
  }
  const unsigned long long sums[4] = {in_m, in_t, sum_m, sum_t};
  const unsigned top_m = wave_max(hd_m), top_t = wave_max(hd_t);
  if (lane == 0) { top[0][threadIdx.x >> 6] = top_m; top[1][threadIdx.x >> 6] = top_t; }
  workgroup_add<4>(part, sums, m->sums, CVH_SCORE_WITHIN_M);   // (its barrier also publishes `top`)
  if (threadIdx.x < 2) {
    unsigned t = 0;
    for (int v = 0; v < kWaves; ++v) t = top[threadIdx.x][v] > t ? top[threadIdx.x][v] : t;
    if (t) atomicMax((unsigned *)(m->sums + CVH_SCORE_HD2_M + threadIdx.x), t);   // the word's low half
  }
}

}  // namespace

hipError_t cvh_launch_score(const CvhIoMember *cols, unsigned col_grid, const CvhIoMember *rows, unsigned row_grid, int nmem, int max_w,
                            int invert, unsigned tol2, hipStream_t s)
{
  const int lds_cols = max_w <= CVH_REINIT_LDS_COLS ? max_w : CVH_REINIT_LDS_COLS;
  hipLaunchKernelGGL(score_class_kernel, dim3(col_grid), dim3(CVH_BLOCK), 0, s, cols, nmem, invert);
  hipLaunchKernelGGL(score_surface_kernel, dim3(col_grid), dim3(CVH_BLOCK), 0, s, cols, nmem);
  hipLaunchKernelGGL(score_columns_kernel, dim3(col_grid), dim3(CVH_BLOCK), 0, s, cols, nmem);
  hipLaunchKernelGGL(score_rows_kernel, dim3(row_grid), dim3(CVH_BLOCK), (size_t)lds_cols * 2 * sizeof(unsigned), s, rows, nmem, tol2);
  return hipGetLastError();
}
