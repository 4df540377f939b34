// energy_kernels.hip — the Chan-Sandberg-Vese functional of the current level set, term by term (gfx950; include/chanvese_hip.h,
// "Energy").  Batch kernels over io_run.hip's member table like the ones in pyramid_kernels.hip and colour_kernels.hip: ONE grid serves N
// members of any mix of shapes and channel counts, a member owning the workgroups first .. first + nblk - 1; the single form launches the
// same kernels with a table of one member.  Table fields: src the level set (doubles), src2 the CvhState whose c1 / c2 are the means of
// that level set (the context's own block, or the one energy_run.hip had the init-sum kernels fill), plane[] the planes, dst the
// member's item rows (its workspace), sums a row of CVH_ENERGY_ROW doubles: [0] eps, read; [1 ..] the results, written.
// Pass 1, energy_terms_kernel -- streaming, 8 + C bytes per pixel: a member is cut into ITEMS of CVH_ENERGY_BAND rows x CVH_ENERGY_COLS
// columns, a wave takes an item at a time, a lane owns two adjacent columns of it and marches down the band with u(r-1), u(r), u(r+1)
// of both in registers -- every value of u is loaded once per band, plus the band's two halo rows and the item's two halo columns.  The
// x-neighbours of a lane's pair are its own other pixel and the adjacent lanes' (DPP wave shifts); lanes 0 and 63 take the item's halo
// column.  Replicate border: every load address is clamped into the plane, so a pixel's missing neighbour IS the pixel itself and no
// load leaves the buffers; pixels behind the last column or row are computed from clamped values and add exact zeros.  (I - c)^2 is
// looked up: 2 C tables of 256 doubles in LDS, built by every workgroup from its member's means.
// Determinism: an item's sums are added lane by lane down the band, then over the wave by wave_sum's fixed tree, and stored as the
// item's row -- whichever wave of whichever grid took the item.  Pass 2, energy_reduce_kernel, one workgroup per member, adds the rows
// in an order the member's shape alone fixes.  No atomics, no dependence on the grid, the arrival order or the other members.
// Arithmetic as the header states it: IEEE divide and sqrt, the device's atan (csv_device.h, heaviside_strict), no contraction.
#include "csv_device.h"
#include "io_device.h"

namespace {

using namespace cvh_dev;

typedef v2d v2d_a8 __attribute__((aligned(8)));                  // a row of doubles starts at a multiple of 8 bytes, not always of 16
typedef unsigned short u16_any __attribute__((aligned(1)));
typedef CVH_GLOBAL const double *gdoubles_in;

constexpr int kSlots = CVH_ENERGY_SLOTS;   // an item's row: length, area, fit_in[3], fit_out[3] (unused channels: zeros)

struct Pair { double a, b; };

// u(r, ca) and u(r, ca + 1) of a row, both columns clamped to w - 1: one 16-byte load where the row has two columns
__device__ __forceinline__ Pair load_pair(gdoubles_in row, int ca, int w)
{
  if (w < 2) { const double v = row[0]; return {v, v}; }
  const int base = ca < w - 2 ? ca : w - 2;
  const v2d p = *(CVH_GLOBAL const v2d_a8 *)(row + base);
  return {ca <= w - 2 ? p.x : p.y, p.y};
}

// the two bytes of a plane's row at the same clamped columns
__device__ __forceinline__ void load_bytes(gbytes_in row, int ca, int w, int &ia, int &ib)
{
  if (w < 2) { ia = ib = row[0]; return; }
  const int base = ca < w - 2 ? ca : w - 2;
  const unsigned v = *(CVH_GLOBAL const u16_any *)(row + base);
  ib = (int)(v >> 8);
  ia = ca <= w - 2 ? (int)(v & 0xffu) : ib;
}

// delta_eps (src/main.cpp:204-210), reference rounding
__device__ __forceinline__ double delta_strict(double x, double eps) { return eps / (kPi * (eps * eps + x * x)); }

template <int C>
__device__ __forceinline__ void terms_of_member(const CvhIoMember *m, const double *lut)
{
  const int h = m->h, w = m->w;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double eps = ((const double *)m->sums)[0];
  const gdoubles_in u = (gdoubles_in)m->src;
  const gbytes_in plane[3] = {(gbytes_in)m->plane[0], (gbytes_in)m->plane[1], (gbytes_in)m->plane[2]};
  double *rows = (double *)m->dst;
  const unsigned pieces = ((unsigned)w + CVH_ENERGY_COLS - 1) / CVH_ENERGY_COLS;
  const unsigned items = cvh_energy_items(h, w);
  const unsigned nwaves = m->nblk * (CVH_BLOCK / 64);
  for (unsigned it = (blockIdx.x - m->first) * (CVH_BLOCK / 64) + wave; it < items; it += nwaves) {
    const int band = (int)(it / pieces), piece = (int)(it - (unsigned)band * pieces);
    const int r0 = band * CVH_ENERGY_BAND, r1 = min(r0 + CVH_ENERGY_BAND, h);
    const int cp = piece * CVH_ENERGY_COLS, ca = cp + 2 * lane;
    const bool va = ca < w, vb = ca + 1 < w;
    // the item's halo column of this lane: lane 63 the one to the right, the others (lane 0 uses it) the one to the left
    const int chalo = lane == 63 ? min(cp + CVH_ENERGY_COLS, w - 1) : max(cp - 1, 0);
    double acc[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) acc[s] = 0.0;
    Pair up = load_pair(u + (size_t)max(r0 - 1, 0) * w, ca, w);
    Pair cur = load_pair(u + (size_t)r0 * w, ca, w);
    double halo = u[(size_t)r0 * w + chalo];
    for (int r = r0; r < r1; ++r) {
      const size_t below = (size_t)min(r + 1, h - 1) * w;
      const Pair dn = load_pair(u + below, ca, w);
      const double halo_dn = u[below + chalo];
      int ia[C], ib[C];
#pragma unroll
      for (int k = 0; k < C; ++k) load_bytes(plane[k] + (size_t)r * w, ca, w, ia[k], ib[k]);
      const double left_a = from_left_lane(cur.b, halo), right_b = from_right_lane(cur.a, halo);
      const double ux[2] = {cur.a, cur.b};
      const double gx[2] = {(cur.b - left_a) * 0.5, (right_b - cur.a) * 0.5};
      const double gy[2] = {(dn.a - up.a) * 0.5, (dn.b - up.b) * 0.5};
      const bool valid[2] = {va, vb};
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const double hv = heaviside_strict(ux[p], eps), omh = 1 - hv;
        const double len = delta_strict(ux[p], eps) * sqrt(gx[p] * gx[p] + gy[p] * gy[p]);
        acc[0] += valid[p] ? len : 0.0;
        acc[1] += valid[p] ? hv : 0.0;
#pragma unroll
        for (int k = 0; k < C; ++k) {
          const int I = p ? ib[k] : ia[k];
          acc[2 + k] += valid[p] ? lut[(2 * k) * 256 + I] * hv : 0.0;
          acc[2 + CVH_MAX_CHANNELS + k] += valid[p] ? lut[(2 * k + 1) * 256 + I] * omh : 0.0;
        }
      }
      up = cur; cur = dn; halo = halo_dn;
    }
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      const double t = wave_sum(acc[s]);
      if (lane == 0) rows[(size_t)it * kSlots + s] = t;
    }
  }
}

__global__ void __launch_bounds__(CVH_BLOCK) energy_terms_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ double lut[2 * CVH_MAX_CHANNELS * 256];   // [2 k] (v - c1_k)^2, [2 k + 1] (v - c2_k)^2, v = 0 .. 255
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const CvhState *st = (const CvhState *)m->src2;
  static_assert(CVH_BLOCK == 256, "a thread builds the tables' entries of one byte value");
  for (int k = 0; k < m->C; ++k) {
    const double v = (double)threadIdx.x, d1 = v - st->c1[k], d2 = v - st->c2[k];
    lut[(2 * k) * 256 + threadIdx.x] = d1 * d1;
    lut[(2 * k + 1) * 256 + threadIdx.x] = d2 * d2;
  }
  __syncthreads();
  if (m->C == 1) terms_of_member<1>(m, lut);
  else terms_of_member<3>(m, lut);
}

// One workgroup per member: thread t adds the rows t, t + 256, ... in that order, block_reduce's fixed tree adds the threads.  The
// means the terms were taken with go out beside them.
__global__ void __launch_bounds__(CVH_BLOCK) energy_reduce_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ double sred[4 * kSlots];
  const CvhIoMember *m = tab + blockIdx.x;
  const double *rows = (const double *)m->dst;
  double *out = (double *)m->sums;
  const unsigned items = cvh_energy_items(m->h, m->w);
  double acc[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) acc[s] = 0.0;
  for (unsigned it = threadIdx.x; it < items; it += CVH_BLOCK) {
#pragma unroll
    for (int s = 0; s < kSlots; ++s) acc[s] += rows[(size_t)it * kSlots + s];
  }
  const double total = block_reduce<kSlots>(acc, sred);
  const int tid = threadIdx.x;
  if (tid < kSlots) out[1 + tid] = total;
  const CvhState *st = (const CvhState *)m->src2;
  if (tid >= 64 && tid < 64 + 2 * CVH_MAX_CHANNELS) {
    const int j = tid - 64;
    out[1 + kSlots + j] = j < CVH_MAX_CHANNELS ? st->c1[j] : st->c2[j - CVH_MAX_CHANNELS];
  }
}

}  // namespace

// workgroups of a member in the term pass: a wave takes an item per trip
unsigned cvh_energy_blocks(int h, int w)
{
  const unsigned b = (cvh_energy_items(h, w) + CVH_BLOCK / 64 - 1) / (CVH_BLOCK / 64);
  return b > 2048 ? 2048 : (b < 1 ? 1 : b);
}

hipError_t cvh_launch_energy(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(energy_terms_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(energy_reduce_kernel, dim3((unsigned)nmem), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}
