// multiphase_kernels.hip — four-phase (Vese-Chan) iteration of TWO level sets (gfx950, wave64; include/chanvese_hip.h, "Four phases").
//
// Step kernel: march_device.h's marching wave over BOTH level sets.  An item is a strip of g.strip_rows rows x CVH_MARCH_COLS columns;
// the rows of the next group of four are requested while the current group is computed.  A double of phi1 / phi2 is read once per
// iteration apart from a strip's three halo columns and three halo rows, and written once: 32 + C bytes per pixel.
// Per pixel: H_eps of the OLD pair (the other level set's blends the region term), the two updates, H_eps of the NEW pair (the sums
// the next iteration's means are taken from).  FAST: the far-field series / table form of H_eps chosen per wave and row.
// Sums: a lane adds its pixels down the strip, wave_sum's fixed tree adds the lanes, lane 0 stores the ITEM's row.  The partition into
// items is a function of the shape alone (cvh_mp_geometry), the finalise kernel -- ONE workgroup -- adds the rows in an order the
// shape alone fixes: no atomics, nothing depends on the grid, on timing or on the order workgroups arrive in.
// Finalise: next means, the two norms, the trace row, the iteration count and the stop flag, into the pair's state block.  Every
// workgroup of every launch reads the flag first and returns where it is set: launches enqueued behind a stop write nothing.
#include "io_device.h"
#include "march_device.h"

using namespace cvh_dev;

namespace {

typedef CVH_GLOBAL const double *gdoubles_in;
typedef CVH_GLOBAL double *gdoubles_out;

constexpr int R = 4;   // rows per group = rows in flight per level set

// H_eps(x).  FAST: 1/2 + the centred value of wave_math.h, the far-field series where every pixel of the wave's row is in the far field,
// else the table form.  Only lanes that own a pixel vote (`owner`): the choice is then a function of the row's stored values alone,
// the same in the step kernel (which holds phi + d in registers) and in a later sums pass over what it stored.
// (Per wave ROW, by ballot, where the localised kernels choose per pixel: here no sum has to be the same bits in two workgroups.)
template <bool FAST, class F>
__device__ __forceinline__ double heaviside(double x, bool owner, const F &a, const FarCoef &fc, const double *satan)
{
  if (!FAST) return heaviside_strict(x, a.eps);
  if (__builtin_amdgcn_ballot_w64(owner && fabs(x) < fc.thr) == 0ull) return 0.5 + heaviside_centred_far(x, fc);
  return 0.5 + heaviside_centred_near(x, a.inv_eps, satan);
}

// the pixel's contribution to the sums of a pair with Heavisides h1, h2
template <int C>
__device__ __forceinline__ void add_pixel(double (&acc)[cvh_mp_nsums(C)], double h1, double h2, const double (&f)[C])
{
  const double g1 = 1 - h1, g2 = 1 - h2;
  const double wt[4] = {h1 * h2, h1 * g2, g1 * h2, g1 * g2};
#pragma unroll
  for (int ab = 0; ab < 4; ++ab) {
    acc[ab] += wt[ab];
#pragma unroll
    for (int k = 0; k < C; ++k) acc[4 + ab * C + k] += f[k] * wt[ab];
  }
}

typedef const CVH_CONSTANT CvhMpArgs *mp_table;

// STEP: one iteration and the sums of the new pair; else the sums of the pair read alone (the call's initial sums, cvh_multiphase_means).
// tab: the members of the launch; a workgroup finds its own through the prefix block counts `first`.  The body is mp_wave_body.inc.
template <int C, bool FAST, bool STEP>
__global__ __launch_bounds__(CVH_BLOCK) void mp_wave_kernel(const CvhMpArgs *tab, int nmem, int parity)
{
  constexpr bool TABLE = true;
  const CVH_CONSTANT CvhMpArgs &a = ((mp_table)tab)[march_member((mp_table)tab, nmem, [](const CVH_CONSTANT CvhMpArgs &m) { return m.first; })];
#include "mp_wave_body.inc"
}

// ONE pair, its record by value: what a call with one pair launches -- the single call's kernel as it was before the batch existed
// (reads u[0][.], writes u[1][.], no prefix count, no mirror of the state block)
template <int C, bool FAST, bool STEP>
__global__ __launch_bounds__(CVH_BLOCK) void mp_wave_kernel_one(const CvhMpArgs a)
{
  constexpr bool TABLE = false;
  constexpr int parity = 0;
#include "mp_wave_body.inc"
}

// ONE workgroup per member: thread t adds the items' rows t, t + 256, ... in that order, block_reduce's fixed tree adds the threads; thread 0
// writes the pair's state block and (TABLE) its mirror in the leader's state table.  is_init: the sums are of the pair the call starts from (or
// reads): the means alone.
template <int C, bool TABLE, class Rec>
__device__ __forceinline__ void mp_finalize_body(const Rec &a, int is_init)
{
  constexpr int NS = cvh_mp_nsums(C);
  __shared__ double sred[4 * NS];
  __shared__ double sfin[NS];
  CvhMpState *st = a.st;
  if (!is_init && st->run.stopped) return;
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  for (int it = threadIdx.x; it < a.g.nitems; it += CVH_BLOCK) {
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] += a.partials[(size_t)it * NS + s];
  }
  const double total = block_reduce<NS>(acc, sred);
  if (threadIdx.x < NS) sfin[threadIdx.x] = total;
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!is_init) {
    const double nrm1 = sqrt(sfin[4 + 4 * C]), nrm2 = sqrt(sfin[5 + 4 * C]);
    const int t = st->run.steps_done;   // index of the iteration just executed
    if (a.trace && t < a.trace_cap) {
      double *row = a.trace + (size_t)t * (4 * C + 2);
      for (int ab = 0; ab < 4; ++ab)
        for (int k = 0; k < C; ++k) row[ab * C + k] = st->c[ab][k];   // the means that iteration used
      row[4 * C] = nrm1;
      row[4 * C + 1] = nrm2;
    }
    st->norm[0] = nrm1;
    st->norm[1] = nrm2;
    st->run.steps_done = t + 1;
    if (nrm1 <= a.stop[0] && nrm2 <= a.stop[1]) st->run.stopped = 1;   // after the update, as src/main.cpp:1000
  } else {
    st->norm[0] = st->norm[1] = 0.0;
    st->run.steps_done = 0;
    st->run.stopped = 0;
  }
  for (int ab = 0; ab < 4; ++ab)
    for (int k = 0; k < C; ++k) st->c[ab][k] = sfin[4 + ab * C + k] / sfin[ab];
  if (!TABLE) return;
  CvhMpState *mirror = a.st_mirror;   // (this thread's own stores, read back)
  mirror->run = st->run;
  mirror->norm[0] = st->norm[0];
  mirror->norm[1] = st->norm[1];
  for (int ab = 0; ab < 4; ++ab)
    for (int k = 0; k < C; ++k) mirror->c[ab][k] = st->c[ab][k];
}

template <int C>
__global__ __launch_bounds__(CVH_BLOCK) void mp_finalize_kernel(const CvhMpArgs *tab, int is_init) { mp_finalize_body<C, true>(((mp_table)tab)[blockIdx.x], is_init); }
template <int C>
__global__ __launch_bounds__(CVH_BLOCK) void mp_finalize_kernel_one(const CvhMpArgs a, int is_init) { mp_finalize_body<C, false>(a, is_init); }

__device__ __forceinline__ unsigned label_of(double u1, double u2) { return (((float)u1 > 0.0f) ? 1u : 0u) | (((float)u2 > 0.0f) ? 2u : 0u); }

// label = mask(phi1) + 2 mask(phi2), mask as io_kernels.hip's mask kernel takes it ((float)u > 0): a lane reads 16 doubles of each level
// set and writes 16 bytes to the caller's buffer (any alignment)
__global__ void __launch_bounds__(CVH_BLOCK) mp_labels_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const size_t n = m->n, pieces = n / 16;
  const size_t t0 = (size_t)(blockIdx.x - m->first) * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  const gdoubles_in u1 = (gdoubles_in)m->src, u2 = (gdoubles_in)m->src2;
  const gbytes_out out = (gbytes_out)m->dst;
  for (size_t q = t0; q < pieces; q += stride) {
    CVH_GLOBAL const v2d *p1 = (CVH_GLOBAL const v2d *)(u1 + 16 * q), *p2 = (CVH_GLOBAL const v2d *)(u2 + 16 * q);
    unsigned wds[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const v2d a1 = p1[2 * i], b1 = p1[2 * i + 1], a2 = p2[2 * i], b2 = p2[2 * i + 1];
      wds[i] = label_of(a1.x, a2.x) | (label_of(a1.y, a2.y) << 8) | (label_of(b1.x, b2.x) << 16) | (label_of(b1.y, b2.y) << 24);
    }
    store16_any(out + 16 * q, make_uint4(wds[0], wds[1], wds[2], wds[3]));
  }
  for (size_t q = pieces * 16 + t0; q < n; q += stride) out[q] = (uint8_t)label_of(u1[q], u2[q]);
}

template <bool STEP>
hipError_t launch_wave(const CvhMpArgs *tab, int nmem, unsigned grid_, int parity, int channels, int fast, hipStream_t s, const CvhMpArgs *one)
{
  const dim3 grid(grid_), block(CVH_BLOCK);
  if (one) {
    if (channels == 1) {
      if (fast) hipLaunchKernelGGL((mp_wave_kernel_one<1, true, STEP>), grid, block, 0, s, *one);
      else hipLaunchKernelGGL((mp_wave_kernel_one<1, false, STEP>), grid, block, 0, s, *one);
    } else {
      if (fast) hipLaunchKernelGGL((mp_wave_kernel_one<3, true, STEP>), grid, block, 0, s, *one);
      else hipLaunchKernelGGL((mp_wave_kernel_one<3, false, STEP>), grid, block, 0, s, *one);
    }
    return hipGetLastError();
  }
  if (channels == 1) {
    if (fast) hipLaunchKernelGGL((mp_wave_kernel<1, true, STEP>), grid, block, 0, s, tab, nmem, parity);
    else hipLaunchKernelGGL((mp_wave_kernel<1, false, STEP>), grid, block, 0, s, tab, nmem, parity);
  } else {
    if (fast) hipLaunchKernelGGL((mp_wave_kernel<3, true, STEP>), grid, block, 0, s, tab, nmem, parity);
    else hipLaunchKernelGGL((mp_wave_kernel<3, false, STEP>), grid, block, 0, s, tab, nmem, parity);
  }
  return hipGetLastError();
}

}  // namespace

// The partition of a plane into items: a strip is one item of cvh_march_rows rows
CvhMpGeom cvh_mp_geometry(int h, int w)
{
  CvhMpGeom g;
  g.nwc = (w + CVH_MARCH_COLS - 1) / CVH_MARCH_COLS;
  g.strip_rows = cvh_march_rows(h, g.nwc);
  g.nstrips = (h + g.strip_rows - 1) / g.strip_rows;
  g.nitems = g.nstrips * g.nwc;   // (< 2^28 / (8 * 61) + ...: the host has refused planes of 2^28 pixels)
  g.grid = (unsigned)((g.nitems + CVH_BLOCK / 64 - 1) / (CVH_BLOCK / 64));
  return g;
}

hipError_t cvh_launch_mp_sums(const CvhMpArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhMpArgs *one)
{
  return launch_wave<false>(tab, nmem, grid, parity, channels, fast, s, one);
}

hipError_t cvh_launch_mp_step(const CvhMpArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhMpArgs *one)
{
  return launch_wave<true>(tab, nmem, grid, parity, channels, fast, s, one);
}

hipError_t cvh_launch_mp_finalize(const CvhMpArgs *tab, int nmem, int channels, int is_init, hipStream_t s, const CvhMpArgs *one)
{
  if (one) {
    if (channels == 1) hipLaunchKernelGGL(mp_finalize_kernel_one<1>, dim3(1), dim3(CVH_BLOCK), 0, s, *one, is_init);
    else hipLaunchKernelGGL(mp_finalize_kernel_one<3>, dim3(1), dim3(CVH_BLOCK), 0, s, *one, is_init);
    return hipGetLastError();
  }
  if (channels == 1) hipLaunchKernelGGL(mp_finalize_kernel<1>, dim3((unsigned)nmem), dim3(CVH_BLOCK), 0, s, tab, is_init);
  else hipLaunchKernelGGL(mp_finalize_kernel<3>, dim3((unsigned)nmem), dim3(CVH_BLOCK), 0, s, tab, is_init);
  return hipGetLastError();
}

hipError_t cvh_launch_mp_labels(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(mp_labels_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}
