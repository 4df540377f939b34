// march_device.h — the marching wave of the four-phase and localised step kernels (gfx950, wave64): a wave owns a strip of rows x
// CVH_MARCH_COLS (61) columns and marches down it, lane l on column 61 wc - 2 + l with u(r-1), u(r), u(r+1) in registers.  The four-wide
// footprint of the curvature along a row -- columns c-2 .. c+1 -- comes from lane moves alone, so lanes 0, 1 and 63 only carry halo
// columns and lanes 2 .. 62 produce pixels.  FAST: wave_math.h's forms; STRICT: the op-by-op forms of the reference (src/main.cpp).
// What a kernel loads, how far ahead, and which form of H_eps it picks is its own.
#pragma once
#include "csv_device.h"
#include "wave_math.h"

namespace cvh_dev {

// a wave's place in the plane: strip and wave-column of its item, the lane's column (clamped: replicate border, no load leaves the
// buffers) and whether the lane owns pixels
struct MarchLane { int lane, strip, wc, s0, s1, col, colc; bool valid; };

__device__ __forceinline__ MarchLane march_lane(long long item, int nwc, int strip_rows, int h, int w)
{
  MarchLane m;
  m.lane = threadIdx.x & 63;
  m.strip = (int)(item / nwc);
  m.wc = (int)(item - (long long)m.strip * nwc);
  m.s0 = m.strip * strip_rows;
  m.s1 = min(m.s0 + strip_rows, h);
  m.col = CVH_MARCH_COLS * m.wc - 2 + m.lane;
  m.colc = clampi(m.col, 0, w - 1);
  m.valid = m.lane >= 2 && m.lane <= 62 && m.col < w;
  return m;
}

// The member table of a launch is read in the constant address space: nothing writes it while a kernel runs, and a record chosen by
// blockIdx alone is wave-uniform, so its fields arrive in scalar loads -- as the fields of a by-value kernel argument do.
#define CVH_CONSTANT __attribute__((address_space(4)))

// the member whose section of the grid holds this workgroup: first(tab[i]) is ascending, first(tab[0]) == 0 (as io_member; wave-uniform)
template <class A, class First>
__device__ __forceinline__ int march_member(const CVH_CONSTANT A *tab, int nmem, First first)
{
  int lo = 0, hi = nmem - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first(tab[mid]) <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the second atan table into LDS (uniform: every thread of the workgroup arrives).  F: a CvhFrontArgs in any address space
template <class F>
__device__ __forceinline__ void stage_atan2(double *satan, const F &f)
{
  const double *tab = f.atan2_tab;
  for (int q = threadIdx.x; q < CVH_ATAN2_N; q += CVH_BLOCK) satan[q] = tab[q];
  __syncthreads();
}

template <class F>
__device__ __forceinline__ FarCoef far_coef_of(const F &f) { return {f.far_k[0], f.far_k[1], f.far_k[2], f.far_k[3], f.far_k[4], f.far_thr}; }

// ny of row r - 1 from u(r - 2), u(r - 1), u(r)
template <bool FAST>
__device__ __forceinline__ double ny_of(double um2, double um, double u0)
{
  return FAST ? normalised4(u0, um2, um + um) : normalised<false>(u0 - um, central(um2, u0));
}

// ny of the row above a strip, from u(s0 - 2) (read only off the plane's first row), u(s0 - 1), u(s0), u(s0 + 1).  kappa_y(0, .) = 0
// (src/main.cpp:372): on the plane's first row it is that row's own ny, by the very expression the row uses, so that ny - ny_prev is
// an exact zero there
template <bool FAST, class Above>
__device__ __forceinline__ double ny_above(int s0, Above um2, double um, double u0, double up)
{
  if (s0 == 0) return ny_of<FAST>(um, u0, up);
  return ny_of<FAST>(um2(), um, u0);
}

// curvature of one level set at the lane's pixel of this row; ny_prev moves on.  fx = (col <= 0) ? 0 : 1: kappa_x(., 0) = 0 (:371)
template <bool FAST>
__device__ __forceinline__ double march_curvature(double um, double u0, double up, double &ny_prev, double fx, int col)
{
  const double uw = from_left_lane(u0, u0), ue = from_right_lane(u0, u0);
  double nx, ny, kappa;
  if (FAST) {
    const double u2 = u0 + u0;
    nx = normalised4(ue, uw, u2);
    ny = normalised4(up, um, u2);
    kappa = __builtin_fma(nx - from_left_lane(nx, 0.0), fx, ny - ny_prev);
  } else {
    nx = normalised<false>(ue - u0, central(uw, ue));   // :365-366
    ny = normalised<false>(up - u0, central(um, up));   // :367-368
    const double nxl = from_left_lane(nx, 0.0);
    const double kx = (col <= 0) ? 0.0 : nx - nxl;      // :371
    kappa = kx + (ny - ny_prev);                        // :372-373
  }
  ny_prev = ny;
  return kappa;
}

// The edge-weighted forms (geodesic_kernels.hip): the normal is scaled by g at its own pixel before the backward differences,
// Gx = g nx, Gy = g ny (one rounding each), and gy_prev -- Gy of the row above -- moves on where ny_prev does above.
// Gy of the row above a strip: g_above() is g(s0 - 1, .), read only off the plane's first row, where the row's own Gy -- g0 ny, by the
// very expression the row uses -- makes Gy - gy_prev an exact zero
template <bool FAST, class Above, class GAbove>
__device__ __forceinline__ double gy_above(int s0, Above um2, GAbove g_above, double um, double u0, double up, double g0)
{
  if (s0 == 0) return g0 * ny_of<FAST>(um, u0, up);
  return g_above() * ny_of<FAST>(um2(), um, u0);
}

template <bool FAST>
__device__ __forceinline__ double march_curvature_weighted(double um, double u0, double up, double g, double &gy_prev, double fx, int col)
{
  const double uw = from_left_lane(u0, u0), ue = from_right_lane(u0, u0);
  double gx, gy, kappa;
  if (FAST) {
    const double u2 = u0 + u0;
    gx = g * normalised4(ue, uw, u2);
    gy = g * normalised4(up, um, u2);
    kappa = __builtin_fma(gx - from_left_lane(gx, 0.0), fx, gy - gy_prev);
  } else {
    gx = g * normalised<false>(ue - u0, central(uw, ue));
    gy = g * normalised<false>(up - u0, central(um, up));
    const double gxl = from_left_lane(gx, 0.0);
    const double kx = (col <= 0) ? 0.0 : gx - gxl;
    kappa = kx + (gy - gy_prev);
  }
  gy_prev = gy;
  return kappa;
}

// dt (mu kappa - nu + F / C) delta_eps(u0), folded as the one-level-set step folds it (:985, :992).  eps2 = eps * eps comes in, taken
// once per kernel: squared in here, the FAST three-channel four-phase kernel spilled scalar registers (profiles/march_refactor)
template <bool FAST>
__device__ __forceinline__ double march_update(double kappa, double F, double u0, double alpha, double beta, double gamma, double eps, double eps2, double dk1)
{
  if (FAST) return __builtin_fma(kappa, alpha, __builtin_fma(F, beta, gamma)) * rcp_refined(inv_delta_eps(u0, eps2, dk1));
  const double ud = kappa * alpha + F * beta + gamma;
  return ud * (eps / (kPi * (eps2 + u0 * u0)));
}

// the wave's sum of x by wave_sum's fixed tree into *dst: halo lanes and lanes behind the last column add nothing, lane 0 stores
__device__ __forceinline__ void march_store_sum(const MarchLane &m, double x, double *dst)
{
  const double t = wave_sum(m.valid ? x : 0.0);
  if (m.lane == 0) *dst = t;
}

}  // namespace cvh_dev
