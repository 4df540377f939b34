// pyramid_kernels.hip — coarse-to-fine runs (gfx950): the planes of a fine context averaged 2 x 2 into a coarse one, and the level set of a
// coarse context replicated 2 x 2 into a fine one (include/chanvese_hip.h, "Coarse-to-fine").  Batch kernels over io_run.hip's member
// table like the ones in io_kernels.hip and init_kernels.hip: ONE grid serves N pairs of any mix of shapes and channel counts, a pair
// owning the workgroups first .. first + nblk - 1; the single-pair entry points launch the same kernels with a table of one member.
// Pure streaming, no LDS staging: every fine byte is read once, every level-set value is read once and written four times.
#include "io_device.h"

namespace {

typedef unsigned long long v2q __attribute__((ext_vector_type(2)));   // two doubles moved as integers: a copy never touches a NaN's payload
typedef v2q v2q_a8 __attribute__((aligned(8)));                        // a row of doubles starts at a multiple of 8 bytes, not always of 16

// 8 fine bytes of the upper row (x: four of them, then y) and the 8 below them -> (a + b + c + d + 2) >> 2 of the four 2 x 2 blocks,
// two output bytes per word pair: 16-bit fields hold the sums (<= 1022)
__device__ __forceinline__ unsigned avg_pairs(unsigned x, unsigned y)
{
  const unsigned m = 0x00ff00ffu;
  const unsigned s = (x & m) + ((x >> 8) & m) + (y & m) + ((y >> 8) & m) + 0x00020002u;
  const unsigned r = (s >> 2) & m;
  return (r | (r >> 8)) & 0xffffu;
}
__device__ __forceinline__ unsigned avg_word(unsigned x0, unsigned x1, unsigned y0, unsigned y1) { return avg_pairs(x0, y0) | (avg_pairs(x1, y1) << 16); }

// Restrict: coarse(r, c) = (f(r0, c0) + f(r0, c1) + f(r1, c0) + f(r1, c1) + 2) >> 2 with r0 = 2r, r1 = min(2r + 1, h2 - 1), c0 = 2c,
// c1 = min(2c + 1, w2 - 1), for every plane of N pairs; sum p and sum p^2 of the coarse planes are added to the member's sums as the
// ingest adds them (exact integers).  A lane produces 16 coarse pixels per trip from two 32-byte runs of fine bytes -- four 16-byte
// loads, one 16-byte store, at any byte address (a row starts wherever the width puts it).  The coarse columns behind a row's last
// whole run -- at most 16, the clamped one of an odd width among them -- go byte by byte in one lane.  5 bytes per coarse pixel and plane.
__global__ void __launch_bounds__(CVH_BLOCK) pyramid_restrict_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const int C = m->C;
  const unsigned hc = (unsigned)m->h, wc = (unsigned)m->w, hf = (unsigned)m->h2, wf = (unsigned)m->w2;
  const unsigned full = wf / 32, per_row = full + (16 * full < wc ? 1u : 0u);
  const size_t items = (size_t)hc * per_row;
  const size_t t0 = (size_t)(blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  const gbytes_out plane[3] = {(gbytes_out)m->plane[0], (gbytes_out)m->plane[1], (gbytes_out)m->plane[2]};
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < C; ++k) {
    const gbytes_in src = (gbytes_in)m->src + (size_t)k * m->src_stride;
    const gbytes_out dst = plane[k];
    unsigned s1 = 0, s2 = 0;
    int pending = 0;
    for (size_t t = t0; t < items; t += stride) {
      const unsigned r = (unsigned)(t / per_row), j = (unsigned)(t - (size_t)r * per_row);
      const unsigned r1 = 2 * r + 1 < hf ? 2 * r + 1 : hf - 1;
      const gbytes_in up = src + (size_t)(2 * r) * wf, lo = src + (size_t)r1 * wf;
      const gbytes_out out = dst + (size_t)r * wc;
      if (j < full) {
        const uint4 a0 = load16_any(up + 32 * j), a1 = load16_any(up + 32 * j + 16), b0 = load16_any(lo + 32 * j), b1 = load16_any(lo + 32 * j + 16);
        const uint4 o = make_uint4(avg_word(a0.x, a0.y, b0.x, b0.y), avg_word(a0.z, a0.w, b0.z, b0.w), avg_word(a1.x, a1.y, b1.x, b1.y),
                                   avg_word(a1.z, a1.w, b1.z, b1.w));
        store16_any(out + 16 * j, o);
        add_bytes(o, s1, s2);
      } else {
        for (unsigned c = 16 * full; c < wc; ++c) {
          const unsigned c0 = 2 * c, c1 = 2 * c + 1 < wf ? 2 * c + 1 : wf - 1;
          const unsigned x = ((unsigned)up[c0] + up[c1] + lo[c0] + lo[c1] + 2u) >> 2;
          out[c] = (uint8_t)x; s1 += x; s2 += x * x;
        }
      }
      if (++pending == kFlushPieces) { flush(acc + 2 * k, s1, s2); pending = 0; }
    }
    flush(acc + 2 * k, s1, s2);
  }
  add_sums(acc, C, m->sums);
}

// Prolong: fine(r, c) = coarse(r >> 1, c >> 1), bit for bit, for N pairs; the member's h x w are the FINE grid, the coarse one is
// ((h + 1) / 2, (w + 1) / 2).  A lane reads a 16-byte piece of a coarse row (two values) and writes each value twice into two fine rows
// with 16-byte stores; the last piece of a row whose duplicates an odd fine width drops, or which holds one value only, goes value by
// value, and an odd fine height drops the second row.  40 bytes per coarse pixel.  A member's first workgroup also clears what a new run
// clears (reset_run_impl), exactly as io_checkerboard_kernel: the four run words of its state block and the chain-mode sum set behind the
// current one.
__global__ void __launch_bounds__(CVH_BLOCK) pyramid_prolong_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const unsigned wg = blockIdx.x - m->first;
  if (wg == 0) {
    if (threadIdx.x < 4) ((CVH_GLOBAL int *)m->state_zero)[threadIdx.x] = 0;
    if (threadIdx.x < 64) ((CVH_GLOBAL long long *)m->chain_zero)[threadIdx.x] = 0;
  }
  const unsigned hf = (unsigned)m->h, wf = (unsigned)m->w, hc = (hf + 1) / 2, wc = (wf + 1) / 2;
  const unsigned per_row = (wc + 1) / 2;
  const size_t items = (size_t)hc * per_row;
  const size_t t0 = (size_t)wg * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  CVH_GLOBAL const unsigned long long *uc = (CVH_GLOBAL const unsigned long long *)m->src;
  CVH_GLOBAL unsigned long long *uf = (CVH_GLOBAL unsigned long long *)m->dst;
  for (size_t t = t0; t < items; t += stride) {
    const unsigned r = (unsigned)(t / per_row), p = (unsigned)(t - (size_t)r * per_row);
    CVH_GLOBAL const unsigned long long *in = uc + (size_t)r * wc;
    CVH_GLOBAL unsigned long long *out0 = uf + (size_t)(2 * r) * wf;
    const bool second = 2 * r + 1 < hf;
    if (4 * p + 3 < wf) {   // (then coarse column 2p + 1 exists and so do the four fine columns)
      const v2q ab = *(CVH_GLOBAL const v2q_a8 *)(in + 2 * p);
      const v2q aa = {ab.x, ab.x}, bb = {ab.y, ab.y};
      *(CVH_GLOBAL v2q_a8 *)(out0 + 4 * p) = aa;
      *(CVH_GLOBAL v2q_a8 *)(out0 + 4 * p + 2) = bb;
      if (second) {
        *(CVH_GLOBAL v2q_a8 *)(out0 + wf + 4 * p) = aa;
        *(CVH_GLOBAL v2q_a8 *)(out0 + wf + 4 * p + 2) = bb;
      }
    } else {
      for (unsigned c = 2 * p; c < 2 * p + 2 && c < wc; ++c) {
        const unsigned long long v = in[c];
        for (unsigned fc = 2 * c; fc < 2 * c + 2 && fc < wf; ++fc) {
          out0[fc] = v;
          if (second) out0[wf + fc] = v;
        }
      }
    }
  }
}

unsigned capped_blocks(size_t items)
{
  const size_t b = items / CVH_BLOCK + 1;
  return (unsigned)(b > 2048 ? 2048 : b);
}

}  // namespace

// items of a pair in the restrict kernel: an item is 16 coarse pixels of a row, or the row's tail (the kernel's hc * per_row)
size_t cvh_restrict_items(int fine_h, int fine_w)
{
  const unsigned wc = ((unsigned)fine_w + 1) / 2, full = (unsigned)fine_w / 32;
  return (size_t)(((unsigned)fine_h + 1) / 2) * (full + (16 * full < wc ? 1u : 0u));
}

// items of a pair in the prolong kernel: an item is two coarse pixels of a row
size_t cvh_prolong_items(int fine_h, int fine_w)
{
  const unsigned wc = ((unsigned)fine_w + 1) / 2;
  return (size_t)(((unsigned)fine_h + 1) / 2) * ((wc + 1) / 2);
}

// workgroups of a pair in the two kernels: a lane takes an item per trip
unsigned cvh_restrict_blocks(int fine_h, int fine_w) { return capped_blocks(cvh_restrict_items(fine_h, fine_w)); }
unsigned cvh_prolong_blocks(int fine_h, int fine_w) { return capped_blocks(cvh_prolong_items(fine_h, fine_w)); }

hipError_t cvh_launch_restrict(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(pyramid_restrict_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_prolong(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(pyramid_prolong_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}
