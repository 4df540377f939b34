// geodesic_kernels.hip — edge-weighted (geodesic) Chan-Vese iteration of ONE level set with global means (gfx950, wave64;
// include/chanvese_hip.h, "Edge-weighted length").
//
// Step kernel: march_device.h's marching wave, as the four-phase kernel runs it, over one level set.  An item is a strip of
// g.strip_rows rows x CVH_MARCH_COLS columns (the four-phase partition, cvh_mp_geometry); the rows of the next group of four are
// requested while the current group is computed.  Per pixel and iteration a double of u is read and written once, C image bytes and
// the 2 bytes of the edge plane are read: 18 + C bytes.  The wave carries Gy = g ny of the previous row where the unweighted march
// carries ny, and takes Gx = g nx of its left neighbour by the lane move (march_curvature_weighted).
// Sums: sum H, sum I_k H and sum d^2 of the NEW level set per item, wave_sum's fixed tree over the lanes, lane 0 stores the item's
// row; the finalise kernel -- ONE workgroup -- adds the rows in an order the shape alone fixes.  No atomics.  The outside means are
// complements: sum I_k and the pixel count do not depend on the level set and come with the record.
// Finalise: next means, the norm, the trace row, the iteration count and the stop flag into the member's state block.  Every workgroup
// of every launch reads the flag first and returns where it is set.
#include "io_device.h"
#include "march_device.h"

using namespace cvh_dev;

namespace {

typedef CVH_GLOBAL const double *gdoubles_in;
typedef CVH_GLOBAL double *gdoubles_out;
typedef CVH_GLOBAL const uint16_t *gwords_in;

constexpr int R = 4;   // rows per group = rows in flight

// H_eps(x), the form chosen per wave and row by the row's own pixels, exactly as the four-phase kernel chooses it (multiphase_kernels.hip):
// the choice is the same in the step kernel, which holds u + d in registers, and in a later sums pass over what it stored
template <bool FAST, class F>
__device__ __forceinline__ double heaviside(double x, bool owner, const F &a, const FarCoef &fc, const double *satan)
{
  if (!FAST) return heaviside_strict(x, a.eps);
  if (__builtin_amdgcn_ballot_w64(owner && fabs(x) < fc.thr) == 0ull) return 0.5 + heaviside_centred_far(x, fc);
  return 0.5 + heaviside_centred_near(x, a.inv_eps, satan);
}

typedef const CVH_CONSTANT CvhGeoArgs *geo_table;

// STEP: one iteration and the sums of the new level set; else the sums of the level set read alone (the call's initial sums)
template <int C, bool FAST, bool STEP>
__global__ __launch_bounds__(CVH_BLOCK) void geo_wave_kernel(const CvhGeoArgs *tab, int nmem, int parity)
{
  constexpr bool TABLE = true;
  const CVH_CONSTANT CvhGeoArgs &a = ((geo_table)tab)[march_member((geo_table)tab, nmem, [](const CVH_CONSTANT CvhGeoArgs &m) { return m.first; })];
#include "geo_wave_body.inc"
}

// ONE member, its record by value: what a call with one member launches
template <int C, bool FAST, bool STEP>
__global__ __launch_bounds__(CVH_BLOCK) void geo_wave_kernel_one(const CvhGeoArgs a)
{
  constexpr bool TABLE = false;
  constexpr int parity = 0;
#include "geo_wave_body.inc"
}

// ONE workgroup per member: thread t adds the items' rows t, t + 256, ... in that order, block_reduce's fixed tree adds the threads;
// thread 0 writes the member's state block and (TABLE) its mirror.  is_init: the sums are of the level set the call starts from
template <int C, bool TABLE, class Rec>
__device__ __forceinline__ void geo_finalize_body(const Rec &a, int is_init)
{
  constexpr int NS = cvh_geo_nsums(C);
  __shared__ double sred[4 * NS];
  __shared__ double sfin[NS];
  CvhGeoState *st = a.st;
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
    const double nrm = sqrt(sfin[1 + C]);
    const int t = st->run.steps_done;   // index of the iteration just executed
    if (a.trace && t < a.trace_cap) {
      double *row = a.trace + (size_t)t * (2 * C + 1);
      for (int k = 0; k < C; ++k) { row[k] = st->c1[k]; row[C + k] = st->c2[k]; }   // the means that iteration used
      row[2 * C] = nrm;
    }
    st->norm = nrm;
    st->run.steps_done = t + 1;
    if (nrm <= a.stop) st->run.stopped = 1;   // after the update
  } else {
    st->norm = 0.0;
    st->run.steps_done = 0;
    st->run.stopped = 0;
  }
  for (int k = 0; k < C; ++k) {
    st->c1[k] = sfin[1 + k] / sfin[0];
    st->c2[k] = (a.sum_img[k] - sfin[1 + k]) / (a.npix - sfin[0]);
  }
  if (!TABLE) return;
  CvhGeoState *mirror = a.st_mirror;   // (this thread's own stores, read back)
  mirror->run = st->run;
  mirror->norm = st->norm;
  for (int k = 0; k < C; ++k) { mirror->c1[k] = st->c1[k]; mirror->c2[k] = st->c2[k]; }
}

template <int C>
__global__ __launch_bounds__(CVH_BLOCK) void geo_finalize_kernel(const CvhGeoArgs *tab, int is_init) { geo_finalize_body<C, true>(((geo_table)tab)[blockIdx.x], is_init); }
template <int C>
__global__ __launch_bounds__(CVH_BLOCK) void geo_finalize_kernel_one(const CvhGeoArgs a, int is_init) { geo_finalize_body<C, false>(a, is_init); }

template <bool STEP>
hipError_t launch_wave(const CvhGeoArgs *tab, int nmem, unsigned grid_, int parity, int channels, int fast, hipStream_t s, const CvhGeoArgs *one)
{
  const dim3 grid(grid_), block(CVH_BLOCK);
  if (one) {
    if (channels == 1) {
      if (fast) hipLaunchKernelGGL((geo_wave_kernel_one<1, true, STEP>), grid, block, 0, s, *one);
      else hipLaunchKernelGGL((geo_wave_kernel_one<1, false, STEP>), grid, block, 0, s, *one);
    } else {
      if (fast) hipLaunchKernelGGL((geo_wave_kernel_one<3, true, STEP>), grid, block, 0, s, *one);
      else hipLaunchKernelGGL((geo_wave_kernel_one<3, false, STEP>), grid, block, 0, s, *one);
    }
    return hipGetLastError();
  }
  if (channels == 1) {
    if (fast) hipLaunchKernelGGL((geo_wave_kernel<1, true, STEP>), grid, block, 0, s, tab, nmem, parity);
    else hipLaunchKernelGGL((geo_wave_kernel<1, false, STEP>), grid, block, 0, s, tab, nmem, parity);
  } else {
    if (fast) hipLaunchKernelGGL((geo_wave_kernel<3, true, STEP>), grid, block, 0, s, tab, nmem, parity);
    else hipLaunchKernelGGL((geo_wave_kernel<3, false, STEP>), grid, block, 0, s, tab, nmem, parity);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t cvh_launch_geo_sums(const CvhGeoArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhGeoArgs *one)
{
  return launch_wave<false>(tab, nmem, grid, parity, channels, fast, s, one);
}

hipError_t cvh_launch_geo_step(const CvhGeoArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhGeoArgs *one)
{
  return launch_wave<true>(tab, nmem, grid, parity, channels, fast, s, one);
}

hipError_t cvh_launch_geo_finalize(const CvhGeoArgs *tab, int nmem, int channels, int is_init, hipStream_t s, const CvhGeoArgs *one)
{
  if (one) {
    if (channels == 1) hipLaunchKernelGGL(geo_finalize_kernel_one<1>, dim3(1), dim3(CVH_BLOCK), 0, s, *one, is_init);
    else hipLaunchKernelGGL(geo_finalize_kernel_one<3>, dim3(1), dim3(CVH_BLOCK), 0, s, *one, is_init);
    return hipGetLastError();
  }
  if (channels == 1) hipLaunchKernelGGL(geo_finalize_kernel<1>, dim3((unsigned)nmem), dim3(CVH_BLOCK), 0, s, tab, is_init);
  else hipLaunchKernelGGL(geo_finalize_kernel<3>, dim3((unsigned)nmem), dim3(CVH_BLOCK), 0, s, tab, is_init);
  return hipGetLastError();
}
