// morph_kernels.hip — mask morphology by a disk and mask starts (cvh_get_mask_morph*, cvh_morph_levelset*, cvh_init_mask*;
// include/chanvese_hip.h "Mask morphology"; gfx950).  A dilation by D(r2) = {dx^2 + dy^2 <= r2} accepts a pixel iff its exact squared
// Euclidean distance to the set is <= r2: the reinitialisation's separable transform (reinit_kernels.hip), thresholded and bounded by the
// radius.  Everything is integer and every launch is ONE grid over N members of mixed shapes (CvhIoMember, cvh_internal.h; the member table
// and the per-member parameters are read with wave-uniform indices, i.e. through the scalar cache); the launches are ordered by their kernel
// boundaries alone -- no workgroup waits for another, no atomic, no floating-point arithmetic.
//   1. morph_bits_kernel     the start set as band words: the plane is cut into bands of 32 rows, a lane owns one column of one band and
//                            packs its 32 pixels into one word (bit r = row r of the band is set) -- from the level set by cvh_get_mask's
//                            rule, or from the byte plane the cleaning launches left.
//   2. morph_columns_kernel  per pass.  A lane owns the same column of the same band: the nearest set row above and below from its own word
//                            by clz / ctz, and where the band has none from the words of the bands above / below (the reinitialisation's
//                            FIX-UP, here cut off at root = floor(sqrt(r2)) rows: farther rows cannot matter).  Writes the vertical
//                            distance g as one 16-bit word per pixel, 0xffff where it exceeds root.
//   3. morph_rows_kernel     per pass.  The same lane builds the word of the result: pixel (i, j) is accepted iff some |k| <= root has
//                            g(i, j + k) != none and k^2 + g(i, j + k)^2 <= r2 (32-bit: k <= root <= 65535 and g <= 65534).  A pixel of
//                            the set has g = 0 and is accepted without a search; the others make at most min(root, w - 1) trips and stop at
//                            the first hit.  The row's distances come from global memory whatever the width: the lanes of a wave read
//                            64 neighbouring 16-bit words per trip.
//      An erosion is the same pass on the complement WITHIN THE PLANE (rows past the last band's end and everything outside the plane
//      belong to neither set): the column launch complements the words it reads, the row launch the word it writes.  Open and close are
//      two passes; the second reads the first's words behind a kernel boundary.
//   4. morph_emit_kernel     the result as 0/1 bytes at any byte address, or as level-set doubles (inside / outside, selected bit for bit):
//                            16 pixels per lane and trip, written in 16-byte pieces; a mask start reads the caller's bytes (nonzero = set)
//                            instead of band words.  A member's first workgroup of a level-set write clears what a new run clears (as
//                            io_checkerboard_kernel).
#include "io_device.h"

namespace {

constexpr unsigned kNone = 0xffffu;   // no set pixel of the column within root rows

// rows of band b that exist, as a bit mask
__device__ __forceinline__ unsigned band_rows(int b, int h)
{
  const int rows = h - b * CVH_REINIT_BAND;
  return rows >= 32 ? 0xffffffffu : ((1u << rows) - 1u);
}

// the workgroups of a member in launches 1 - 3: band-major, 256 columns each (reinit_kernels.hip's)
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

__global__ void __launch_bounds__(CVH_BLOCK) morph_bits_kernel(const CvhIoMember *tab, int nmem, int from_levelset, int invert)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const int h = m->h, w = m->w;
  const ColumnSlot s = column_slot(m);
  if (!s.live) return;
  const int r0 = s.band * CVH_REINIT_BAND, rows = h - r0 < CVH_REINIT_BAND ? h - r0 : CVH_REINIT_BAND;
  unsigned word = 0;
  if (from_levelset) {   // (wave-uniform: the call's)
    CVH_GLOBAL const double *u = (CVH_GLOBAL const double *)m->src;
    for (int r = 0; r < rows; ++r) word |= (((float)u[(size_t)(r0 + r) * w + s.col] > 0.0f) ? 1u : 0u) << r;   // cvh_get_mask's rule
    if (invert) word = ~word & band_rows(s.band, h);
  } else {
    const gbytes_in f = (gbytes_in)m->src2;
    for (int r = 0; r < rows; ++r) word |= (f[(size_t)(r0 + r) * w + s.col] ? 1u : 0u) << r;
  }
  ((CVH_GLOBAL unsigned *)m->plane[0])[(size_t)s.band * w + s.col] = word;
}

__global__ void __launch_bounds__(CVH_BLOCK) morph_columns_kernel(const CvhIoMember *tab, const CvhMorphPar *par, int nmem, int from, int complement)
{
  const int mi = io_member(tab, nmem);
  const CvhIoMember *m = tab + mi;
  const int h = m->h, w = m->w, nbands = (h + CVH_REINIT_BAND - 1) / CVH_REINIT_BAND;
  const int root = (int)(par[mi].root < 65535u ? par[mi].root : 65535u);
  const ColumnSlot s = column_slot(m);
  if (!s.live) return;
  CVH_GLOBAL const unsigned *bits = (CVH_GLOBAL const unsigned *)m->plane[from];
  CVH_GLOBAL unsigned short *g = (CVH_GLOBAL unsigned short *)m->plane[2];
  const unsigned flip = complement ? 0xffffffffu : 0u;
  const unsigned cls = (bits[(size_t)s.band * w + s.col] ^ flip) & band_rows(s.band, h);
  const int r0 = s.band * CVH_REINIT_BAND, rows = h - r0 < CVH_REINIT_BAND ? h - r0 : CVH_REINIT_BAND;
  // fix-up: the nearest set row above and below the band (-1: none within root rows of any row of the band)
  int above = -1, below = -1;
  for (int b = s.band - 1; b >= 0 && above < 0 && r0 - (b * CVH_REINIT_BAND + 31) <= root; --b) {
    const unsigned c = bits[(size_t)b * w + s.col] ^ flip;   // (bands above the last one are whole)
    if (c) above = b * CVH_REINIT_BAND + 31 - __builtin_clz(c);
  }
  for (int b = s.band + 1; b < nbands && below < 0 && b * CVH_REINIT_BAND - (r0 + rows - 1) <= root; ++b) {
    const unsigned c = (bits[(size_t)b * w + s.col] ^ flip) & band_rows(b, h);
    if (c) below = b * CVH_REINIT_BAND + __builtin_ctz(c);
  }
  for (int r = 0; r < rows; ++r) {
    const int i = r0 + r;
    const unsigned up = cls & (0xffffffffu >> (31 - r)), down = cls >> r;   // rows <= r / rows >= r of the band
    const int ia = up ? r0 + 31 - __builtin_clz(up) : above, ib = down ? i + __builtin_ctz(down) : below;
    int best = root + 1;
    if (ia >= 0 && i - ia < best) best = i - ia;
    if (ib >= 0 && ib - i < best) best = ib - i;
    g[(size_t)i * w + s.col] = (unsigned short)(best <= root ? (unsigned)best : kNone);   // (best <= h - 1 <= 65534)
  }
}

__global__ void __launch_bounds__(CVH_BLOCK) morph_rows_kernel(const CvhIoMember *tab, const CvhMorphPar *par, int nmem, int to, int complement)
{
  const int mi = io_member(tab, nmem);
  const CvhIoMember *m = tab + mi;
  const int h = m->h, w = m->w;
  const unsigned r2 = par[mi].r2, root = par[mi].root;
  const ColumnSlot s = column_slot(m);
  if (!s.live) return;
  CVH_GLOBAL const unsigned short *g = (CVH_GLOBAL const unsigned short *)m->plane[2];
  const int r0 = s.band * CVH_REINIT_BAND, rows = h - r0 < CVH_REINIT_BAND ? h - r0 : CVH_REINIT_BAND;
  const int j = s.col;
  const unsigned reach = (unsigned)(j > w - 1 - j ? j : w - 1 - j), kmax = root < reach ? root : reach;
  unsigned word = 0;
  for (int r = 0; r < rows; ++r) {
    CVH_GLOBAL const unsigned short *grow = g + (size_t)(r0 + r) * w;
    bool hit = grow[j] != kNone;   // a distance is stored only where it is <= root, and root^2 <= r2
    for (unsigned k = 1; !hit && k <= kmax; ++k) {
      const unsigned rem = r2 - k * k;   // (k <= root: no wrap)
      if ((unsigned)j >= k) {
        const unsigned v = grow[j - (int)k];
        hit = v != kNone && v * v <= rem;
      }
      if (!hit && (unsigned)j + k < (unsigned)w) {
        const unsigned v = grow[j + (int)k];
        hit = v != kNone && v * v <= rem;
      }
    }
    word |= (hit ? 1u : 0u) << r;
  }
  if (complement) word = ~word & band_rows(s.band, h);
  ((CVH_GLOBAL unsigned *)m->plane[to])[(size_t)s.band * w + s.col] = word;
}

template <bool FROM_BYTES, bool TO_LEVELSET>
__global__ void __launch_bounds__(CVH_BLOCK) morph_emit_kernel(const CvhIoMember *tab, const CvhMorphPar *par, int nmem)
{
  const int mi = io_member(tab, nmem);
  const CvhIoMember *m = tab + mi;
  const int wg = (int)(blockIdx.x - m->first);
  const size_t n = m->n, pieces = n / 16, w = (size_t)m->w;
  const size_t t0 = (size_t)wg * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  const gbytes_in src = (gbytes_in)m->src;
  CVH_GLOBAL const unsigned *words = (CVH_GLOBAL const unsigned *)m->plane[0];
  const gbytes_out out = (gbytes_out)m->dst;
  CVH_GLOBAL double *u = (CVH_GLOBAL double *)m->dst;
  const double inside = par[mi].inside, outside = par[mi].outside;
  if (TO_LEVELSET && wg == 0) {   // the device's share of a new run (reset_run_impl)
    if (threadIdx.x < 4) ((CVH_GLOBAL int *)m->state_zero)[threadIdx.x] = 0;
    if (threadIdx.x < 64) ((CVH_GLOBAL long long *)m->chain_zero)[threadIdx.x] = 0;
  }
  auto set_at = [&](size_t p) -> bool {
    if (FROM_BYTES) return src[p] != 0;
    const size_t i = p / w, jj = p - i * w;
    return (words[(i >> 5) * w + jj] >> (i & 31)) & 1u;
  };
  for (size_t q = t0; q < pieces; q += stride) {
    unsigned set = 0;   // bit b: pixel 16 q + b
    if (FROM_BYTES) {
      const uint4 v = load16_any(src + 16 * q);
      const unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int b = 0; b < 16; ++b) set |= (((wds[b >> 2] >> (8 * (b & 3))) & 0xffu) ? 1u : 0u) << b;
    } else {
      size_t i = (16 * q) / w, jj = 16 * q - i * w;
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        set |= ((words[(i >> 5) * w + jj] >> (i & 31)) & 1u) << b;
        if (++jj == w) { jj = 0; ++i; }
      }
    }
    if (TO_LEVELSET) {
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const v2d o = {(set >> (2 * b)) & 1u ? inside : outside, (set >> (2 * b + 1)) & 1u ? inside : outside};
        ((CVH_GLOBAL v2d *)u)[8 * q + b] = o;
      }
    } else {
      unsigned o[4];
#pragma unroll
      for (int d = 0; d < 4; ++d)
        o[d] = ((set >> (4 * d)) & 1u) | (((set >> (4 * d + 1)) & 1u) << 8) | (((set >> (4 * d + 2)) & 1u) << 16) | (((set >> (4 * d + 3)) & 1u) << 24);
      store16_any(out + 16 * q, make_uint4(o[0], o[1], o[2], o[3]));
    }
  }
  for (size_t p = pieces * 16 + t0; p < n; p += stride) {
    const bool in = set_at(p);
    if (TO_LEVELSET) u[p] = in ? inside : outside;
    else out[p] = in ? 1 : 0;
  }
}

}  // namespace

hipError_t cvh_launch_morph_bits(const CvhIoMember *cols, int nmem, unsigned col_grid, bool from_levelset, int invert, hipStream_t s)
{
  hipLaunchKernelGGL(morph_bits_kernel, dim3(col_grid), dim3(CVH_BLOCK), 0, s, cols, nmem, from_levelset ? 1 : 0, invert ? 1 : 0);
  return hipGetLastError();
}

hipError_t cvh_launch_morph_passes(const CvhIoMember *cols, const CvhMorphPar *par, int nmem, unsigned col_grid, int npass, const bool *complement,
                                   hipStream_t s)
{
  for (int k = 0; k < npass; ++k) {
    hipLaunchKernelGGL(morph_columns_kernel, dim3(col_grid), dim3(CVH_BLOCK), 0, s, cols, par, nmem, k & 1, complement[k] ? 1 : 0);
    hipLaunchKernelGGL(morph_rows_kernel, dim3(col_grid), dim3(CVH_BLOCK), 0, s, cols, par, nmem, (k + 1) & 1, complement[k] ? 1 : 0);
  }
  return hipGetLastError();
}

hipError_t cvh_launch_morph_emit(const CvhIoMember *tab, const CvhMorphPar *par, int nmem, unsigned grid, bool from_bytes, bool to_levelset,
                                 hipStream_t s)
{
  if (from_bytes && !to_levelset) return hipErrorInvalidValue;   // (bytes to bytes is a copy: no call asks for it)
  if (from_bytes) hipLaunchKernelGGL((morph_emit_kernel<true, true>), dim3(grid), dim3(CVH_BLOCK), 0, s, tab, par, nmem);
  else if (to_levelset) hipLaunchKernelGGL((morph_emit_kernel<false, true>), dim3(grid), dim3(CVH_BLOCK), 0, s, tab, par, nmem);
  else hipLaunchKernelGGL((morph_emit_kernel<false, false>), dim3(grid), dim3(CVH_BLOCK), 0, s, tab, par, nmem);
  return hipGetLastError();
}
