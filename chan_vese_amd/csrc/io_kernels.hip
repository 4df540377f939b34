// io_kernels.hip — device-memory input and output of contexts and batches of contexts (gfx950): ingest of uint8 images with their sums,
// the plane sums of planes already on the device, the checkerboard level set, mask / level-set / plane egress.  Batch kernels: ONE grid serves N members, a member owning the workgroups
// first .. first + nblk - 1; the member table (CvhIoMember, cvh_internal.h) is read with wave-uniform indices, i.e. through the scalar
// cache.  The single-context entry points launch the same kernels with a table of one member; image_sums_kernel alone takes plain
// arguments (its planes sit on the device: an ingest would only add a copy) and shares the ingest's sums.
#include "io_device.h"

namespace {

// byte `i` (0 .. 11) of the 12 bytes {a, b, c}
__device__ __forceinline__ unsigned byte12(unsigned a, unsigned b, unsigned c, int i)
{
  const unsigned w = i < 4 ? a : (i < 8 ? b : c);
  return (w >> (8 * (i & 3))) & 0xffu;
}

// 48 interleaved bytes (16 pixels x 3 channels, in[0..11]) -> 16 bytes per channel
__device__ __forceinline__ void split3(const unsigned in[12], uint4 out[3])
{
  unsigned o[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {   // pixels 4j .. 4j + 3 are the 12 bytes in[3j .. 3j + 2]
#pragma unroll
    for (int k = 0; k < 3; ++k)
      o[k][j] = byte12(in[3 * j], in[3 * j + 1], in[3 * j + 2], k) | (byte12(in[3 * j], in[3 * j + 1], in[3 * j + 2], k + 3) << 8) |
                (byte12(in[3 * j], in[3 * j + 1], in[3 * j + 2], k + 6) << 16) | (byte12(in[3 * j], in[3 * j + 1], in[3 * j + 2], k + 9) << 24);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = make_uint4(o[k][0], o[k][1], o[k][2], o[k][3]);
}

// 16 bytes per channel -> 48 interleaved bytes
__device__ __forceinline__ void join3(const uint4 in[3], unsigned out[12])
{
  const unsigned p[3][4] = {{in[0].x, in[0].y, in[0].z, in[0].w}, {in[1].x, in[1].y, in[1].z, in[1].w}, {in[2].x, in[2].y, in[2].z, in[2].w}};
#pragma unroll
  for (int d = 0; d < 12; ++d) {
    unsigned v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = 4 * d + b, px = i / 3, k = i % 3;   // byte i of the 48 is channel k of pixel px
      v |= ((p[k][px >> 2] >> (8 * (px & 3))) & 0xffu) << (8 * b);
    }
    out[d] = v;
  }
}

// Ingest: the caller's uint8 bytes become the member's planes, and sum p / sum p^2 of every plane are added to the member's sums as exact
// 64-bit integers (image_sums_kernel's, below: the same adds).  A lane moves 16 pixels per trip; the n % 16 last pixels go byte by
// byte.  Every source byte is read once.
__global__ void __launch_bounds__(CVH_BLOCK) io_ingest_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const int C = m->C;
  const size_t n = m->n, pieces = n / 16;
  const size_t t0 = (size_t)(blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  const gbytes_in src = (gbytes_in)m->src;
  const gbytes_out plane[3] = {(gbytes_out)m->plane[0], (gbytes_out)m->plane[1], (gbytes_out)m->plane[2]};
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  if (m->interleaved && C == 3) {   // (wave-uniform: a member's layout)
    unsigned s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
    int pending = 0;
    for (size_t q = t0; q < pieces; q += stride) {
      const uint4 a = load16_any(src + 48 * q), b = load16_any(src + 48 * q + 16), c = load16_any(src + 48 * q + 32);
      const unsigned in[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
      uint4 out[3];
      split3(in, out);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        store16(plane[k], q, out[k]);
        add_bytes(out[k], s1[k], s2[k]);
      }
      if (++pending == kFlushPieces) {
#pragma unroll
        for (int k = 0; k < 3; ++k) flush(acc + 2 * k, s1[k], s2[k]);
        pending = 0;
      }
    }
    for (size_t q = pieces * 16 + t0; q < n; q += stride) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { const unsigned x = src[3 * q + k]; plane[k][q] = (uint8_t)x; s1[k] += x; s2[k] += x * x; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) flush(acc + 2 * k, s1[k], s2[k]);
  } else {
    for (int k = 0; k < C; ++k) {
      const gbytes_in s = src + (size_t)k * n;
      const gbytes_out d = plane[k];
      unsigned s1 = 0, s2 = 0;
      int pending = 0;
      for (size_t q = t0; q < pieces; q += stride) {
        const uint4 v = load16_any(s + 16 * q);
        store16(d, q, v);
        add_bytes(v, s1, s2);
        if (++pending == kFlushPieces) { flush(acc + 2 * k, s1, s2); pending = 0; }
      }
      for (size_t q = pieces * 16 + t0; q < n; q += stride) { const unsigned x = s[q]; d[q] = (uint8_t)x; s1 += x; s2 += x * x; }
      flush(acc + 2 * k, s1, s2);
    }
  }
  add_sums(acc, C, m->sums);
}

// Per-plane sum(p) and sum(p^2) of planes that already sit on the device (16-byte aligned), as exact 64-bit integers (out[2k],
// out[2k+1]; zeroed by the caller): the region means' sum(I) and, for one channel, the tol-free stop norm of src/main.cpp:950-959 (every
// partial sum of the reference's loop is an integer below 2^53 there, so its result does not depend on the order).
__global__ void __launch_bounds__(CVH_BLOCK) image_sums_kernel(const uint8_t *p0, const uint8_t *p1, const uint8_t *p2, int C, size_t n,
                                                               unsigned long long *out)
{
  const gbytes_in pl[3] = {(gbytes_in)p0, (gbytes_in)p1, (gbytes_in)p2};
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  const size_t pieces = n / 16, stride = (size_t)gridDim.x * CVH_BLOCK, t0 = (size_t)blockIdx.x * CVH_BLOCK + threadIdx.x;
  for (int k = 0; k < C; ++k) {
    unsigned s1 = 0, s2 = 0;
    int pending = 0;
    for (size_t q = t0; q < pieces; q += stride) {
      add_bytes(load16(pl[k], q), s1, s2);
      if (++pending == kFlushPieces) { flush(acc + 2 * k, s1, s2); pending = 0; }
    }
    for (size_t q = pieces * 16 + t0; q < n; q += stride) { const unsigned x = pl[k][q]; s1 += x; s2 += x * x; }
    flush(acc + 2 * k, s1, s2);
  }
  add_sums(acc, C, out);
}

// levelset_checkerboard, src/main.cpp:226-231: sign(sin(pi i/5) * sin(pi j/5)), for N members.  src = the h row factors, src2 = the w
// column factors, both from the host's libm (checkerboard_factors); the product is ONE IEEE multiplication, so the device reproduces
// cvh_levelset_checkerboard_host bit for bit without 8 bytes per pixel crossing PCIe.  dst = the level set.  A member's first workgroup also clears what a new run clears (reset_run_impl):
// the four run words of its state block and the chain-mode sum set behind the current one.
__global__ void __launch_bounds__(CVH_BLOCK) io_checkerboard_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const int h = m->h, w = m->w, wg = (int)(blockIdx.x - m->first), nblk = (int)m->nblk;
  CVH_GLOBAL const double *si = (CVH_GLOBAL const double *)m->src, *sj = (CVH_GLOBAL const double *)m->src2;
  CVH_GLOBAL double *u = (CVH_GLOBAL double *)m->dst;
  if (wg == 0) {
    if (threadIdx.x < 4) ((CVH_GLOBAL int *)m->state_zero)[threadIdx.x] = 0;
    if (threadIdx.x < 64) ((CVH_GLOBAL long long *)m->chain_zero)[threadIdx.x] = 0;
  }
  for (int i = wg; i < h; i += nblk) {
    const double s = si[i];
    for (int j = (int)threadIdx.x; j < w; j += CVH_BLOCK) {
      const double z = s * sj[j];
      u[(size_t)i * w + j] = (z == 0) ? 0.0 : (z < 0 ? -1.0 : 1.0);
    }
  }
}

__device__ __forceinline__ unsigned mask_bit(double u, int invert) { return (((float)u > 0.0f) ? 1u : 0u) ^ (unsigned)invert; }

// mask = ((float)u > 0), optionally inverted (src/main.cpp:395-400), N members -- the one mask kernel, cvh_get_mask's too: a lane reads 16 doubles (two 64-byte row pieces) and writes
// 16 bytes to the caller's buffer (any alignment)
__global__ void __launch_bounds__(CVH_BLOCK) io_mask_kernel(const CvhIoMember *tab, int nmem, int invert)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const size_t n = m->n, pieces = n / 16;
  const size_t t0 = (size_t)(blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  CVH_GLOBAL const double *u = (CVH_GLOBAL const double *)m->src;
  const gbytes_out out = (gbytes_out)m->dst;
  for (size_t q = t0; q < pieces; q += stride) {
    CVH_GLOBAL const v2d *p = (CVH_GLOBAL const v2d *)(u + 16 * q);
    unsigned wds[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const v2d a = p[2 * i], b = p[2 * i + 1];
      wds[i] = mask_bit(a.x, invert) | (mask_bit(a.y, invert) << 8) | (mask_bit(b.x, invert) << 16) | (mask_bit(b.y, invert) << 24);
    }
    store16_any(out + 16 * q, make_uint4(wds[0], wds[1], wds[2], wds[3]));
  }
  for (size_t q = pieces * 16 + t0; q < n; q += stride) out[q] = (uint8_t)mask_bit(u[q], invert);
}

// the member's planes into the caller's interleaved h * w * 3 bytes
__global__ void __launch_bounds__(CVH_BLOCK) io_image_out3_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const size_t n = m->n, pieces = n / 16;
  const size_t t0 = (size_t)(blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  const gbytes_out out = (gbytes_out)m->dst;
  const gbytes_in plane[3] = {(gbytes_in)m->plane[0], (gbytes_in)m->plane[1], (gbytes_in)m->plane[2]};
  for (size_t q = t0; q < pieces; q += stride) {
    uint4 in[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) in[k] = load16(plane[k], q);
    unsigned o[12];
    join3(in, o);
#pragma unroll
    for (int t = 0; t < 3; ++t) store16_any(out + 48 * q + 16 * t, make_uint4(o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]));
  }
  for (size_t q = pieces * 16 + t0; q < n; q += stride) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * q + k] = plane[k][q];
  }
}

// level set out as float, rounded to nearest even (state_narrow_kernel's rule); the context's doubles stay as they are
__global__ void io_narrow_kernel(const double *u, float *out, size_t n)
{
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) out[q] = (float)u[q];
}

}  // namespace

// workgroups of a member of n pixels in a kernel whose lanes move 16 pixels per trip
unsigned cvh_io_blocks(size_t n)
{
  const size_t b = (n / 16 + CVH_BLOCK) / CVH_BLOCK;
  return (unsigned)(b > 2048 ? 2048 : b);
}

unsigned cvh_io_checkerboard_blocks(int h, int w)
{
  const size_t b = ((size_t)h * w + 8191) / 8192;
  const size_t cap = h < 1024 ? h : 1024;
  return (unsigned)(b > cap ? cap : (b < 1 ? 1 : b));
}

hipError_t cvh_launch_io_ingest(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(io_ingest_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_image_sums(const uint8_t *const *planes, int channels, size_t n, unsigned long long *out, hipStream_t s)
{
  const size_t b = (n / 16 + 1 + CVH_BLOCK - 1) / CVH_BLOCK;
  hipLaunchKernelGGL(image_sums_kernel, dim3((unsigned)(b > 1024 ? 1024 : b)), dim3(CVH_BLOCK), 0, s, planes[0], channels > 1 ? planes[1] : nullptr,
                     channels > 2 ? planes[2] : nullptr, channels, n, out);
  return hipGetLastError();
}

hipError_t cvh_launch_io_checkerboard(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(io_checkerboard_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_io_mask(const CvhIoMember *tab, int nmem, unsigned grid, int invert, hipStream_t s)
{
  hipLaunchKernelGGL(io_mask_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem, invert ? 1 : 0);
  return hipGetLastError();
}

hipError_t cvh_launch_io_image_out3(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(io_image_out3_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_io_narrow(const double *u, float *out, size_t n, hipStream_t s)
{
  hipLaunchKernelGGL(io_narrow_kernel, dim3((unsigned)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384)), dim3(256), 0, s, u, out, n);
  return hipGetLastError();
}
