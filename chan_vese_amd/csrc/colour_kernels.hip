// colour_kernels.hip — colour spaces on the device (gfx950): the three planes of a context converted in place between (B, G, R) or
// (R, G, B) and (Y, Cr, Cb) or (Y, U, V), and the luma plane of a three-channel context written into a one-channel context
// (include/chanvese_hip.h, "Colour spaces": all arithmetic in signed 32-bit integers).  Batch kernels over io_run.hip's member table like
// the ones in io_kernels.hip and pyramid_kernels.hip: ONE grid serves N members of any mix of shapes, a member owning the workgroups
// first .. first + nblk - 1; the single forms launch the same kernels with a table of one member.  space, order and inverse are call-wide
// kernel arguments (wave-uniform selects of a few constants in front of the loop).
// Pure streaming, no LDS staging: a lane takes one 16-byte piece -- 16 pixels -- of each of the three planes, computes the 16 pixels from
// byte-extracted words and stores three pieces (convert: 6 bytes per pixel) or one (luma: 4 bytes per pixel).  A lane reads its own
// pieces before it writes them and no other lane touches them, so the in-place conversion needs no ordering.  A plane of h * w bytes that
// is no multiple of 16 ends in a partial piece: its LOAD stays inside the plane's own padding (cvh_create pads every plane of the slab to
// a multiple of 256 bytes, the last one included), its bytes behind h * w count for nothing, and its STORE goes byte by byte, so no byte
// behind h * w is ever written.  The sums of the planes written are the ingest's (io_device.h: exact integers).
#include "io_device.h"

namespace {

constexpr int kHalf = 8192;            // H: 1/2 in 14 fractional bits
constexpr int kDelta = 128 << 14;      // D: the chroma offset

struct ColourCoef {
  int swap;        // forward: plane 0 is B (CVH_ORDER_BGR); inverse: plane 0 takes B
  int yuv;         // the first chroma plane belongs to B - Y (U), the second to R - Y (V); YCrCb: the other way round
  int k1, k2;      // forward: multipliers of the first and the second chroma plane
  int kr, kgb, kgr, kb;   // inverse: R from a(R chroma); G from a(B chroma), a(R chroma); B from a(B chroma)
};

__device__ __forceinline__ ColourCoef colour_coef(int space, int order)
{
  const bool yuv = space == CVH_COLOUR_YUV;
  ColourCoef k;
  k.swap = order == CVH_ORDER_BGR;
  k.yuv = yuv;
  k.k1 = yuv ? 8061 : 11682;
  k.k2 = yuv ? 14369 : 9241;
  k.kr = yuv ? 18678 : 22987;
  k.kgb = yuv ? -6472 : -5636;
  k.kgr = yuv ? -9519 : -11698;
  k.kb = yuv ? 33292 : 29049;
  return k;
}

__device__ __forceinline__ int sat8(int x) { return min(max(x, 0), 255); }

__device__ __forceinline__ int luma_of(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + kHalf) >> 14; }

// one pixel forward: planes (p0, p1, p2) in the caller's order -> (Y, first chroma, second chroma)
__device__ __forceinline__ void forward_px(const ColourCoef &k, int p0, int p1, int p2, int &o0, int &o1, int &o2)
{
  const int r = k.swap ? p2 : p0, b = k.swap ? p0 : p2;
  const int y = luma_of(r, p1, b);
  const int d1 = (k.yuv ? b : r) - y, d2 = (k.yuv ? r : b) - y;
  o0 = y;
  o1 = sat8((d1 * k.k1 + kDelta + kHalf) >> 14);   // (>> of a negative int: the arithmetic shift)
  o2 = sat8((d2 * k.k2 + kDelta + kHalf) >> 14);
}

// one pixel back: (Y, first chroma, second chroma) -> R, G, B in the caller's order
__device__ __forceinline__ void inverse_px(const ColourCoef &k, int y, int p1, int p2, int &o0, int &o1, int &o2)
{
  const int ar = (k.yuv ? p2 : p1) - 128, ab = (k.yuv ? p1 : p2) - 128;
  const int r = sat8(y + ((ar * k.kr + kHalf) >> 14));
  const int g = sat8(y + ((ab * k.kgb + ar * k.kgr + kHalf) >> 14));
  const int b = sat8(y + ((ab * k.kb + kHalf) >> 14));
  o0 = k.swap ? b : r;
  o1 = g;
  o2 = k.swap ? r : b;
}

__device__ __forceinline__ int byte_of(unsigned w, int b) { return (int)((w >> (8 * b)) & 0xffu); }

// the bytes 0 .. keep - 1 of a piece, the others zero (keep = 16: all of it)
__device__ __forceinline__ uint4 keep_bytes(uint4 v, unsigned keep)
{
  unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned left = keep > 4u * i ? keep - 4u * i : 0u;   // bytes of word i that count
    wds[i] = left >= 4 ? wds[i] : (left ? wds[i] & ((1u << (8 * left)) - 1u) : 0u);
  }
  return make_uint4(wds[0], wds[1], wds[2], wds[3]);
}

// piece q of a plane whose last piece may be partial: `keep` of its bytes exist
__device__ __forceinline__ void store_piece(gbytes_out plane, size_t q, uint4 v, unsigned keep)
{
  if (keep == 16) { store16(plane, q, v); return; }
  const unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if ((unsigned)i < keep) plane[16 * q + i] = (uint8_t)byte_of(wds[i >> 2], i & 3);
}

// Convert: the three planes of every member replaced in place, forward or back; sum p and sum p^2 of the new planes are added to the
// member's sums as the ingest adds them.
__global__ void __launch_bounds__(CVH_BLOCK) colour_convert_kernel(const CvhIoMember *tab, int nmem, int space, int order, int inverse)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const ColourCoef k = colour_coef(space, order);
  const size_t n = m->n, pieces = (n + 15) / 16;
  const size_t t0 = (size_t)(blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  const gbytes_out plane[3] = {(gbytes_out)m->plane[0], (gbytes_out)m->plane[1], (gbytes_out)m->plane[2]};
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  unsigned s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
  int pending = 0;
  for (size_t q = t0; q < pieces; q += stride) {
    const uint4 a = load16(plane[0], q), b = load16(plane[1], q), c = load16(plane[2], q);
    const unsigned in[3][4] = {{a.x, a.y, a.z, a.w}, {b.x, b.y, b.z, b.w}, {c.x, c.y, c.z, c.w}};
    unsigned o[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[0][i] = o[1][i] = o[2][i] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int x0, x1, x2;
        if (inverse) inverse_px(k, byte_of(in[0][i], j), byte_of(in[1][i], j), byte_of(in[2][i], j), x0, x1, x2);
        else forward_px(k, byte_of(in[0][i], j), byte_of(in[1][i], j), byte_of(in[2][i], j), x0, x1, x2);
        o[0][i] |= (unsigned)x0 << (8 * j); o[1][i] |= (unsigned)x1 << (8 * j); o[2][i] |= (unsigned)x2 << (8 * j);
      }
    }
    const size_t left = n - 16 * q;
    const unsigned keep = left < 16 ? (unsigned)left : 16u;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const uint4 v = keep_bytes(make_uint4(o[p][0], o[p][1], o[p][2], o[p][3]), keep);
      store_piece(plane[p], q, v, keep);
      add_bytes(v, s1[p], s2[p]);
    }
    if (++pending == kFlushPieces) {
#pragma unroll
      for (int p = 0; p < 3; ++p) flush(acc + 2 * p, s1[p], s2[p]);
      pending = 0;
    }
  }
#pragma unroll
  for (int p = 0; p < 3; ++p) flush(acc + 2 * p, s1[p], s2[p]);
  add_sums(acc, 3, m->sums);
}

// Luma: Y of the three planes at src (src_stride bytes apart) into the member's single plane, with its sums.  The source is only read.
__global__ void __launch_bounds__(CVH_BLOCK) colour_luma_kernel(const CvhIoMember *tab, int nmem, int order)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const bool swap = order == CVH_ORDER_BGR;
  const size_t n = m->n, pieces = (n + 15) / 16;
  const size_t t0 = (size_t)(blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  const gbytes_in src = (gbytes_in)m->src;
  const gbytes_in pr = src + (swap ? 2 * m->src_stride : 0), pg = src + m->src_stride, pb = src + (swap ? 0 : 2 * m->src_stride);
  const gbytes_out dst = (gbytes_out)m->plane[0];
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  unsigned s1 = 0, s2 = 0;
  int pending = 0;
  for (size_t q = t0; q < pieces; q += stride) {
    const uint4 a = load16(pr, q), b = load16(pg, q), c = load16(pb, q);
    const unsigned in[3][4] = {{a.x, a.y, a.z, a.w}, {b.x, b.y, b.z, b.w}, {c.x, c.y, c.z, c.w}};
    unsigned o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[i] |= (unsigned)luma_of(byte_of(in[0][i], j), byte_of(in[1][i], j), byte_of(in[2][i], j)) << (8 * j);
    }
    const size_t left = n - 16 * q;
    const unsigned keep = left < 16 ? (unsigned)left : 16u;
    const uint4 v = keep_bytes(make_uint4(o[0], o[1], o[2], o[3]), keep);
    store_piece(dst, q, v, keep);
    add_bytes(v, s1, s2);
    if (++pending == kFlushPieces) { flush(acc, s1, s2); pending = 0; }
  }
  flush(acc, s1, s2);
  add_sums(acc, 1, m->sums);
}

}  // namespace

// workgroups of a member of n pixels: an item is a 16-byte piece, the partial last one included; CVH_BLOCK lanes take a piece per trip
unsigned cvh_colour_blocks(size_t n)
{
  const size_t b = (n + CVH_COLOUR_BLOCK_PIXELS - 1) / CVH_COLOUR_BLOCK_PIXELS;
  return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

hipError_t cvh_launch_colour_convert(const CvhIoMember *tab, int nmem, unsigned grid, int space, int order, int inverse, hipStream_t s)
{
  hipLaunchKernelGGL(colour_convert_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem, space, order, inverse ? 1 : 0);
  return hipGetLastError();
}

hipError_t cvh_launch_colour_luma(const CvhIoMember *tab, int nmem, unsigned grid, int order, hipStream_t s)
{
  hipLaunchKernelGGL(colour_luma_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem, order);
  return hipGetLastError();
}
