// edge_kernels.hip — the edge plane of "Edge-weighted length" (include/chanvese_hip.h): the Sobel edge map on the member table, and the
// clamped copy of a caller's device buffer (gfx950).
// Edge map: a lane takes a pixel per trip, consecutive lanes consecutive pixels, and reads the 3 x 3 neighbourhood of every source plane
// with the coordinates clamped to the plane (replicate border; no load leaves the planes).  Integer Sobel sums, ONE conversion, two IEEE
// divisions and a round-half-even: every value is a function of the nine bytes per plane and of den alone.
#include "io_device.h"

namespace {

typedef CVH_GLOBAL uint16_t *gwords_out;
typedef CVH_GLOBAL const uint16_t *gwords_in;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(CVH_BLOCK) edge_map_kernel(const CvhIoMember *tab, const double *dens, int nmem)
{
  const int mi = io_member(tab, nmem);
  const CvhIoMember *m = tab + mi;
  const int h = m->h, w = m->w, C = m->w2;
  const size_t n = m->n;
  const double den = dens[mi];
  const gwords_out out = (gwords_out)m->dst;
  const size_t stride = (size_t)m->nblk * CVH_BLOCK;
  for (size_t q = (size_t)(blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x; q < n; q += stride) {
    const int r = (int)(q / (size_t)w), c = (int)(q - (size_t)r * w);
    const size_t r0 = (size_t)clampi(r - 1, 0, h - 1) * w, r1 = (size_t)r * w, r2 = (size_t)clampi(r + 1, 0, h - 1) * w;
    const int cw = clampi(c - 1, 0, w - 1), ce = clampi(c + 1, 0, w - 1);
    int m2 = 0;   // at most 3 * 2 * 1020^2
    for (int k = 0; k < C; ++k) {
      const gbytes_in p = (gbytes_in)m->src + (size_t)k * m->src_stride;
      const int nw = p[r0 + cw], nn = p[r0 + c], ne = p[r0 + ce];
      const int ww = p[r1 + cw], ee = p[r1 + ce];
      const int sw = p[r2 + cw], ss = p[r2 + c], se = p[r2 + ce];
      const int sx = (ne + 2 * ee + se) - (nw + 2 * ww + sw);
      const int sy = (sw + 2 * ss + se) - (nw + 2 * nn + ne);
      m2 += sx * sx + sy * sy;
    }
    out[q] = (uint16_t)rint(32768.0 / (1.0 + (double)m2 / den));
  }
}

__global__ void __launch_bounds__(CVH_BLOCK) edge_clamp_kernel(const uint16_t *src_, uint16_t *dst_, size_t n)
{
  const gwords_in src = (gwords_in)src_;
  const gwords_out dst = (gwords_out)dst_;
  const size_t stride = (size_t)gridDim.x * CVH_BLOCK;
  for (size_t q = (size_t)blockIdx.x * CVH_BLOCK + threadIdx.x; q < n; q += stride) {
    const unsigned v = src[q];
    dst[q] = (uint16_t)(v > CVH_EDGE_ONE ? CVH_EDGE_ONE : v);
  }
}

}  // namespace

// four trips per lane from 1024 pixels on, at most 4096 workgroups
unsigned cvh_edge_blocks(size_t n)
{
  const size_t b = (n + 4 * CVH_BLOCK - 1) / (4 * CVH_BLOCK);
  return (unsigned)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

hipError_t cvh_launch_edge_map(const CvhIoMember *tab, const double *den, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(edge_map_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, den, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_edge_clamp(const uint16_t *src, uint16_t *dst, size_t n, hipStream_t s)
{
  hipLaunchKernelGGL(edge_clamp_kernel, dim3(cvh_edge_blocks(n)), dim3(CVH_BLOCK), 0, s, src, dst, n);
  return hipGetLastError();
}
