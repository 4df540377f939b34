// convex_kernels.hip — primal-dual iteration of the convex relaxation of two-phase Chan-Vese (gfx950, wave64; include/chanvese_hip.h,
// "Convex relaxation").
//
// Step kernel: march_device.h's marching wave over the four-phase partition (cvh_mp_geometry): an item is a strip of g.strip_rows rows x
// CVH_MARCH_COLS columns, the rows of the next group of four are requested while the current group is computed.  A lane holds vbar(r)
// and vbar(r + 1) of its column, takes vbar(r, c + 1) from its right lane and qx'(r, c - 1) from its left lane -- lane 1 computes the
// dual of the halo column for that alone -- and carries qy' of the row above, where the geodesic kernel carries Gy; at a strip's first
// row that value is recomputed from the OLD q and vbar of rows s0 - 1 and s0 (the sets read are not written by this launch).
// Per pixel and iteration: v read and written in place (16 bytes), vbar, qx, qy read from one set and written to the other (48), C image
// bytes, and the 2 bytes of the edge plane where one is used: 64 + C, or 66 + C with an edge plane.
// Sums: sum v', sum I_k v' and sum d^2 per item, wave_sum's fixed tree over the lanes, lane 0 stores the item's row; the finalise kernel
// -- ONE workgroup per member -- adds the rows in an order the shape alone fixes.  No atomics.
// Finalise: the norm, the trace row, the iteration count, the stop flag and -- after every means_every-th iteration -- the next means
// into the member's state block.  Every workgroup of every step launch reads the flag first and returns where it is set.
#include <algorithm>

#include "io_device.h"
#include "march_device.h"

using namespace cvh_dev;

namespace {

typedef CVH_GLOBAL const double *gdoubles_in;
typedef CVH_GLOBAL double *gdoubles_out;
typedef CVH_GLOBAL const uint16_t *gwords_in;

constexpr int R = 4;   // rows per group = rows in flight

// the dual update of one pixel: q + sigma grad vbar, projected onto the disk of radius rho
template <bool FAST>
__device__ __forceinline__ void cvx_dual(double qx, double qy, double dx, double dy, double sigma, double rho, double &px, double &py)
{
  if (FAST) {
    const double tx = __builtin_fma(sigma, dx, qx), ty = __builtin_fma(sigma, dy, qy);
    const double s2 = __builtin_fma(tx, tx, ty * ty);
    const double k = s2 > rho * rho ? rho * rsqrt_refined(s2) : 1.0;   // (s2 > rho^2 >= 0: the root exists)
    px = tx * k; py = ty * k;
    return;
  }
  const double tx = qx + sigma * dx, ty = qy + sigma * dy;
  const double s = sqrt(tx * tx + ty * ty);
  if (s > rho) { const double k = rho / s; px = tx * k; py = ty * k; }
  else { px = tx; py = ty; }
}

// the primal update of one pixel: v + tau (div q' - r), clamped to [0, 1] (a NaN stays a NaN)
template <int C, bool FAST>
__device__ __forceinline__ double cvx_primal(const double (&f)[C], const double (&c1)[C], const double (&c2)[C], const double (&l1)[C],
                                             const double (&l2)[C], double nu, double tau, double div, double v)
{
  double t[C];
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const double a = f[k] - c1[k], b = f[k] - c2[k];
    t[k] = FAST ? __builtin_fma(l1[k], a * a, -(l2[k] * (b * b))) : l1[k] * (a * a) - l2[k] * (b * b);
  }
  double r, x;
  if (C == 1) r = nu + t[0];
  else {
    const double sum = (t[0] + t[C > 1 ? 1 : 0]) + t[C > 2 ? 2 : 0];
    r = FAST ? __builtin_fma(sum, 1.0 / C, nu) : nu + sum / C;
  }
  x = FAST ? __builtin_fma(tau, div - r, v) : v + tau * (div - r);
  return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
}

typedef const CVH_CONSTANT CvhCvxArgs *cvx_table;

// STEP: one iteration and the sums of the new v; else the start: v0, vbar0, q = 0 and the sums of v0
template <int C, bool FAST, bool STEP>
__global__ __launch_bounds__(CVH_BLOCK) void cvx_wave_kernel(const CvhCvxArgs *tab, int nmem, int parity)
{
  constexpr bool TABLE = true;
  const CVH_CONSTANT CvhCvxArgs &a = ((cvx_table)tab)[march_member((cvx_table)tab, nmem, [](const CVH_CONSTANT CvhCvxArgs &m) { return m.first; })];
#include "cvx_wave_body.inc"
}

// ONE member, its record by value: what a call with one member launches
template <int C, bool FAST, bool STEP>
__global__ __launch_bounds__(CVH_BLOCK) void cvx_wave_kernel_one(const CvhCvxArgs a)
{
  constexpr bool TABLE = false;
  constexpr int parity = 0;
#include "cvx_wave_body.inc"
}

// ONE workgroup per member: thread t adds the items' rows t, t + 256, ... in that order, block_reduce's fixed tree adds the threads;
// thread 0 writes the member's state block and (TABLE) its mirror.  is_init: in front of iteration 0 -- the whole block from the sums of
// v0, or, where the member resumes, the run counters alone
template <int C, bool TABLE, class Rec>
__device__ __forceinline__ void cvx_finalize_body(const Rec &a, int is_init)
{
  constexpr int NS = cvh_cvx_nsums(C);
  __shared__ double sred[4 * NS];
  __shared__ double sfin[NS];
  CvhCvxState *st = a.st;
  if (!is_init && st->run.stopped) return;
  const bool sums = !(is_init && a.resume);   // (uniform)
  if (sums) {
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
  }
  if (threadIdx.x != 0) return;
  bool retake = false;
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
    if (nrm <= a.stop) st->run.stopped = 1;   // after the update (a negative stop: never)
    const int since = st->since + 1;
    retake = a.means_every > 0 && since >= a.means_every;
    st->since = retake ? 0 : since;
  } else {
    st->run.steps_done = 0;
    st->run.stopped = 0;
    if (sums) { st->norm = 0.0; st->since = 0; st->pad = 0; retake = true; }
  }
  if (retake) {
    for (int k = 0; k < C; ++k) {
      st->c1[k] = sfin[1 + k] / sfin[0];
      st->c2[k] = (a.sum_img[k] - sfin[1 + k]) / (a.npix - sfin[0]);
    }
  }
  if (!TABLE) return;
  CvhCvxState *mirror = a.st_mirror;   // (this thread's own stores, read back)
  mirror->run = st->run;
  mirror->norm = st->norm;
  mirror->since = st->since;
  for (int k = 0; k < C; ++k) { mirror->c1[k] = st->c1[k]; mirror->c2[k] = st->c2[k]; }
}

template <int C>
__global__ __launch_bounds__(CVH_BLOCK) void cvx_finalize_kernel(const CvhCvxArgs *tab, int is_init) { cvx_finalize_body<C, true>(((cvx_table)tab)[blockIdx.x], is_init); }
template <int C>
__global__ __launch_bounds__(CVH_BLOCK) void cvx_finalize_kernel_one(const CvhCvxArgs a, int is_init) { cvx_finalize_body<C, false>(a, is_init); }

// u = v - 0.5: the level set whose mask is the threshold of v at 1/2
__global__ __launch_bounds__(CVH_BLOCK) void cvx_bake_kernel(const double *v, double *u, size_t n)
{
  for (size_t i = (size_t)blockIdx.x * CVH_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * CVH_BLOCK) u[i] = v[i] - 0.5;
}

template <bool STEP>
hipError_t launch_wave(const CvhCvxArgs *tab, int nmem, unsigned grid_, int parity, int channels, int fast, hipStream_t s, const CvhCvxArgs *one)
{
  const dim3 grid(grid_), block(CVH_BLOCK);
  if (one) {
    if (channels == 1) {
      if (fast) hipLaunchKernelGGL((cvx_wave_kernel_one<1, true, STEP>), grid, block, 0, s, *one);
      else hipLaunchKernelGGL((cvx_wave_kernel_one<1, false, STEP>), grid, block, 0, s, *one);
    } else {
      if (fast) hipLaunchKernelGGL((cvx_wave_kernel_one<3, true, STEP>), grid, block, 0, s, *one);
      else hipLaunchKernelGGL((cvx_wave_kernel_one<3, false, STEP>), grid, block, 0, s, *one);
    }
    return hipGetLastError();
  }
  if (channels == 1) {
    if (fast) hipLaunchKernelGGL((cvx_wave_kernel<1, true, STEP>), grid, block, 0, s, tab, nmem, parity);
    else hipLaunchKernelGGL((cvx_wave_kernel<1, false, STEP>), grid, block, 0, s, tab, nmem, parity);
  } else {
    if (fast) hipLaunchKernelGGL((cvx_wave_kernel<3, true, STEP>), grid, block, 0, s, tab, nmem, parity);
    else hipLaunchKernelGGL((cvx_wave_kernel<3, false, STEP>), grid, block, 0, s, tab, nmem, parity);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t cvh_launch_cvx_start(const CvhCvxArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhCvxArgs *one)
{
  return launch_wave<false>(tab, nmem, grid, parity, channels, fast, s, one);
}

hipError_t cvh_launch_cvx_step(const CvhCvxArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhCvxArgs *one)
{
  return launch_wave<true>(tab, nmem, grid, parity, channels, fast, s, one);
}

hipError_t cvh_launch_cvx_finalize(const CvhCvxArgs *tab, int nmem, int channels, int is_init, hipStream_t s, const CvhCvxArgs *one)
{
  if (one) {
    if (channels == 1) hipLaunchKernelGGL(cvx_finalize_kernel_one<1>, dim3(1), dim3(CVH_BLOCK), 0, s, *one, is_init);
    else hipLaunchKernelGGL(cvx_finalize_kernel_one<3>, dim3(1), dim3(CVH_BLOCK), 0, s, *one, is_init);
    return hipGetLastError();
  }
  if (channels == 1) hipLaunchKernelGGL(cvx_finalize_kernel<1>, dim3((unsigned)nmem), dim3(CVH_BLOCK), 0, s, tab, is_init);
  else hipLaunchKernelGGL(cvx_finalize_kernel<3>, dim3((unsigned)nmem), dim3(CVH_BLOCK), 0, s, tab, is_init);
  return hipGetLastError();
}

hipError_t cvh_launch_cvx_bake(const double *v, double *u, size_t n, hipStream_t s)
{
  const unsigned grid = (unsigned)std::min<size_t>((n + CVH_BLOCK - 1) / CVH_BLOCK, 4096);
  hipLaunchKernelGGL(cvx_bake_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, v, u, n);
  return hipGetLastError();
}
