// localized_kernels.hip — localised Chan-Vese: region means over a window, retaken every iteration (gfx950, wave64;
// include/chanvese_hip.h, "Localised regions").  Three launches per iteration, none waits for another workgroup, no atomics.
//
// ROW pass: a workgroup takes one row segment of CVH_WINDOW_SEGMENT columns and the R columns on either side of it (the span, at most
// 1278 pixels: five consecutive pixels per thread).  A thread reads u and the image bytes of its pixels, forms wq = rint(H_eps(u) 2^40)
// and the products wq f_k, and the workgroup takes the prefix sums of the 1 + C series in LDS (a thread's own five, a wave scan of the
// threads' totals, the four waves' totals); the horizontal window sum of a column is the difference of two prefix entries, so the work
// per pixel does not grow with R.  The sums are unsigned 64-bit integers: a pixel that lies in two segments' spans has the same wq in
// both (the form of H_eps is chosen per PIXEL by its own stored value), and every sum is the same bits in any order.
// STEP kernel: march_device.h's marching wave down a strip of g.strip_rows rows.  The vertical running sums of the 1 + C workspace
// planes live in registers: the strip's start adds the up to 2 R + 1 rows of its first window, every later row adds the row entering
// the window and subtracts the row leaving it -- exact, they are integers.  Beside them u(r-1), u(r), u(r+1) for the curvature, the
// bytes of the image and T_k.  The loads of row r + 1 are issued before row r is computed.  Per pixel: A, S_k -> B, S'_k
// -> the 2 C means (one IEEE division each) -> F -> d; the other buffer of the pair is written, d^2 is added per lane, and at every
// item boundary (g.item_rows rows: a function of the shape alone) wave_sum's fixed tree adds the lanes and lane 0 stores the item's sum.
// The same kernel without the update writes the means and sums of the current level set (cvh_localized_means) or, behind a row pass
// with wq = 1, the planes T_k (once per call).
// FINALISE: one workgroup adds the items in index order (thread t takes t, t + 256, ...; block_reduce's fixed tree), writes the norm,
// the trace row, the count and the stop flag.  Every workgroup of every launch of an iteration reads the flag first and returns where
// it is set: launches enqueued behind a stop write nothing.  The launches of cvh_localized_means and of the planes T_k are not part of a
// run and never read the state block: a stop that an earlier run left there does not concern them.
#include <algorithm>

#include "io_device.h"
#include "march_device.h"

using namespace cvh_dev;

namespace {

typedef CVH_GLOBAL const double *gdoubles_in;
typedef CVH_GLOBAL double *gdoubles_out;
typedef CVH_GLOBAL const unsigned long long *gu64_in;
typedef CVH_GLOBAL unsigned long long *gu64_out;
typedef CVH_GLOBAL const unsigned *gu32_in;
typedef CVH_GLOBAL unsigned *gu32_out;

constexpr int kSeg = CVH_WINDOW_SEGMENT;
constexpr int kSpanMax = kSeg + 2 * CVH_LOC_RADIUS_MAX;
constexpr int kPer = (kSpanMax + CVH_BLOCK - 1) / CVH_BLOCK;   // consecutive pixels of the span a thread takes
constexpr unsigned long long kOne = 1ull << CVH_LOC_FRAC_BITS;
static_assert(kPer * CVH_BLOCK >= kSpanMax, "the workgroup covers the longest span");
static_assert((1 + CVH_MAX_CHANNELS) * (kSpanMax + 1) * 8 + (CVH_ATAN2_N + 1) * 8 + 256 <= 64 * 1024, "the row pass's LDS");

// wq of a pixel: a function of its stored double alone.  FAST: wave_math.h's far-field series from the threshold on, its table form below
// (per PIXEL, where the four-phase kernel votes per wave row: a pixel in two segments' spans must give the same wq in both)
template <bool FAST, class F>
__device__ __forceinline__ unsigned long long weight_of(double x, const F &a, const FarCoef &fc, const double *satan)
{
  double H;
  if (!FAST) H = heaviside_strict(x, a.eps);
  else H = 0.5 + (fabs(x) < fc.thr ? heaviside_centred_near(x, a.inv_eps, satan) : heaviside_centred_far(x, fc));
  const double q = __builtin_rint(H * (double)kOne);
  return (unsigned long long)fmin(fmax(q, 0.0), (double)kOne);   // (a NaN gives 0)
}

// MODE 0: STRICT, 1: FAST, 2: wq = 1 (the sums of the planes alone, for T_k).  IN_RUN: a launch of an iteration of cvh_localized_run, which
// returns where the member's stop flag is set; the other launches (T_k, cvh_localized_means) do not read the state block at all.
// tab: the members of the launch; a workgroup finds its own through the prefix block counts row_first
typedef const CVH_CONSTANT CvhLocArgs *loc_table;

// (Rec: a CvhLocArgs in the constant address space -- a record of the table -- or the by-value argument of the one-member entry point)
// TABLE: the record is one of a table's -- the member's workgroups lie behind `first` others, the buffer read is u[parity].  Else the
// launch is the member's alone, reads u[0] and writes u[1] (the host swaps them per iteration): the parent single-call kernel
template <int C, int MODE, bool IN_RUN, bool TABLE, class Rec>
__device__ __forceinline__ void loc_row_body(const Rec &a, int parity)
{
  const unsigned blk = TABLE ? blockIdx.x - a.row_first : blockIdx.x;
  constexpr int NQ = 1 + C;
  __shared__ unsigned long long pre[NQ][kSpanMax + 1];   // pre[q][i]: the sum of the span's first i entries
  __shared__ unsigned long long wtot[NQ][CVH_BLOCK / 64];
  __shared__ double satan[MODE == 1 ? CVH_ATAN2_N + 1 : 1];
  if (IN_RUN && a.st->run.stopped) return;   // (uniform: before the barriers)
  if (MODE == 1) stage_atan2(satan, a.f);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = a.h, w = a.w, R = a.radius;
  const int r = (int)(blk / (unsigned)a.g.nseg), seg = (int)(blk % (unsigned)a.g.nseg);
  if (r >= h) return;
  const int c0 = seg * kSeg, cend = min(c0 + kSeg, w);
  const int first = max(c0 - R, 0), last = min(cend - 1 + R, w - 1), len = last - first + 1;   // len <= kSpanMax
  const FarCoef fc = far_coef_of(a.f);
  const size_t row = (size_t)r * w, n = (size_t)h * w;
  const gdoubles_in in = (gdoubles_in)(TABLE && parity ? a.u[1] : a.u[0]);
  const gbytes_in plane[CVH_MAX_CHANNELS] = {(gbytes_in)a.img[0], (gbytes_in)a.img[1], (gbytes_in)a.img[2]};

  unsigned long long v[NQ][kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = tid * kPer + j;
    const bool ok = i < len;
    const int col = first + (ok ? i : 0);   // (inside the row)
    unsigned long long wq = 1;
    if (MODE != 2) {
      wq = weight_of<MODE == 1>(in[row + col], a.f, fc, satan);
      if (a.wq_out && ok && col >= c0 && col < cend) ((gu64_out)a.wq_out)[row + col] = wq;
    }
    if (!ok) wq = 0;
    v[0][j] = wq;
#pragma unroll
    for (int k = 0; k < C; ++k) v[1 + k][j] = wq * (unsigned long long)plane[k][row + col];
  }
  // inclusive prefix sums: the thread's own, the wave's threads, the waves
  unsigned long long incl[NQ], mine[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int j = 1; j < kPer; ++j) v[q][j] += v[q][j - 1];
    mine[q] = v[q][kPer - 1];
    unsigned long long s = mine[q];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long t = __shfl_up(s, d, 64);
      if (lane >= d) s += t;
    }
    incl[q] = s;
    if (lane == 63) wtot[q][wave] = s;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    unsigned long long base = incl[q] - mine[q];
    for (int x = 0; x < wave; ++x) base += wtot[q][x];
    if (tid == 0) pre[q][0] = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int i = tid * kPer + j;
      if (i < len) pre[q][i + 1] = base + v[q][j];
    }
  }
  __syncthreads();
  for (int col = c0 + tid; col < cend; col += CVH_BLOCK) {
    const int lo = max(col - R, first) - first, hi = min(col + R, last) - first + 1;   // 0 <= lo < hi <= len
#pragma unroll
    for (int q = 0; q < NQ; ++q) ((gu64_out)a.hw)[(size_t)q * n + row + col] = pre[q][hi] - pre[q][lo];
  }
}

template <int C, int MODE, bool IN_RUN>
__global__ __launch_bounds__(CVH_BLOCK) void loc_row_kernel(const CvhLocArgs *tab, int nmem, int parity)
{
  loc_row_body<C, MODE, IN_RUN, true>(((loc_table)tab)[march_member((loc_table)tab, nmem, [](const CVH_CONSTANT CvhLocArgs &m) { return m.row_first; })], parity);
}

// ONE member, its record by value: what a call with one member launches -- the single call's kernel as it was before the batch
// existed (reads u[0], writes u[1], no prefix count, no mirror of the state block)
template <int C, int MODE, bool IN_RUN>
__global__ __launch_bounds__(CVH_BLOCK) void loc_row_kernel_one(const CvhLocArgs a)
{
  loc_row_body<C, MODE, IN_RUN, false>(a, 0);
}

template <int C, bool FAST, int KIND, bool TABLE, class Rec>
__device__ __forceinline__ void loc_wave_body(const Rec &a, int parity)
{
  constexpr int NQ = 1 + C;
  constexpr bool STEP = KIND == CVH_LOC_STEP, TSUM = KIND == CVH_LOC_TSUM;
  if (STEP && a.st->run.stopped) return;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long witem = (long long)(TABLE ? blockIdx.x - a.wave_first : blockIdx.x) * (CVH_BLOCK / 64) + wave;
  if (witem >= (long long)a.g.nstrips * a.g.nwc) return;
  const int h = a.h, w = a.w, R = a.radius;
  const MarchLane ml = march_lane(witem, a.g.nwc, a.g.strip_rows, h, w);
  const int wc = ml.wc, s0 = ml.s0, s1 = ml.s1, col = ml.col, colc = ml.colc;
  const bool lane_valid = ml.valid;
  const size_t n = (size_t)h * w;
  const double eps = a.f.eps, eps2 = eps * eps;
  const gdoubles_in in = (gdoubles_in)(TABLE && parity ? a.u[1] : a.u[0]);
  const gdoubles_out out = (gdoubles_out)(TABLE && parity ? a.u[0] : a.u[1]);
  const gu64_in hw = (gu64_in)a.hw;
  const gbytes_in plane[CVH_MAX_CHANNELS] = {(gbytes_in)a.img[0], (gbytes_in)a.img[1], (gbytes_in)a.img[2]};
  const int ncols = min(colc + R, w - 1) - max(colc - R, 0) + 1;

  double l1[C], l2[C];
#pragma unroll
  for (int k = 0; k < C; ++k) { l1[k] = a.lambda1[k]; l2[k] = a.lambda2[k]; }

  // the first window of the strip: rows max(s0 - R, 0) .. min(s0 + R, h - 1)
  unsigned long long V[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) V[q] = 0;
  for (int j = max(s0 - R, 0); j <= min(s0 + R, h - 1); ++j) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) V[q] += hw[(size_t)q * n + (size_t)j * w + colc];
  }

  // what row r needs beside the running sums; every index is clamped into the plane, so no load leaves the buffers.  (ONE row ahead,
  // where the four-phase kernel asks for four: a row here is also the 2 (1 + C) sums entering and leaving the window)
  struct RowData { double up; unsigned f[C], T[C]; unsigned long long E[NQ], L[NQ]; };
  auto request = [&](int r, RowData &d) {
    const size_t o = (size_t)clampi(r, 0, h - 1) * w + colc;
    d = RowData{};
    if (STEP) d.up = in[(size_t)clampi(r + 1, 0, h - 1) * w + colc];
    if (!TSUM) {
#pragma unroll
      for (int k = 0; k < C; ++k) { d.f[k] = plane[k][o]; d.T[k] = ((gu32_in)a.tsum)[(size_t)k * n + o]; }
    }
    const bool enter = r + 1 + R < h, leave = r - R >= 0;   // (wave-uniform) the window of row r + 1 against that of row r
    const size_t oe = (size_t)min(r + 1 + R, h - 1) * w + colc, ol = (size_t)max(r - R, 0) * w + colc;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      d.E[q] = enter ? hw[(size_t)q * n + oe] : 0ull;
      d.L[q] = leave ? hw[(size_t)q * n + ol] : 0ull;
    }
  };

  double um = 0.0, u0 = 0.0, nyp = 0.0, acc = 0.0;
  const double fx = (col <= 0) ? 0.0 : 1.0;
  RowData cur;
  if (s0 < s1) request(s0, cur);
  if (STEP && s0 < s1) {
    auto at = [&](int r) -> double { return in[(size_t)clampi(r, 0, h - 1) * w + colc]; };
    um = at(s0 - 1); u0 = at(s0);
    nyp = ny_above<FAST>(s0, [&] { return at(s0 - 2); }, um, u0, cur.up);
  }

  for (int r = s0; r < s1; ++r) {
    RowData nxt;
    const bool more = r + 1 < s1;   // (wave-uniform)
    if (more) request(r + 1, nxt);
    const size_t o = (size_t)r * w + colc;
    if (TSUM) {
      if (lane_valid) {
#pragma unroll
        for (int k = 0; k < C; ++k) ((gu32_out)a.tsum)[(size_t)k * n + o] = (unsigned)V[1 + k];
      }
    } else {
      const int nrows = min(r + R, h - 1) - max(r - R, 0) + 1;
      const unsigned long long A = V[0], B = ((unsigned long long)(nrows * ncols) << CVH_LOC_FRAC_BITS) - A;
      const double Ad = (double)A, Bd = (double)B;
      double F = 0.0;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const unsigned long long S = V[1 + k], Sp = ((unsigned long long)cur.T[k] << CVH_LOC_FRAC_BITS) - S;
        const double c1 = (double)S / Ad, c2 = (double)Sp / Bd;   // IEEE division in both modes: 0 / 0 is NaN
        const double f = (double)cur.f[k];
        F += -l1[k] * ((f - c1) * (f - c1)) + l2[k] * ((f - c2) * (f - c2));
        if (!STEP && lane_valid) {
          if (a.c1_out) ((gdoubles_out)a.c1_out)[(size_t)k * n + o] = c1;
          if (a.c2_out) ((gdoubles_out)a.c2_out)[(size_t)k * n + o] = c2;
          if (a.s_out) ((gu64_out)a.s_out)[(size_t)k * n + o] = S;
        }
      }
      if (!STEP && lane_valid && a.a_out) ((gu64_out)a.a_out)[o] = A;
      if (STEP) {
        const double up = cur.up;
        const double kappa = march_curvature<FAST>(um, u0, up, nyp, fx, col);
        const double d = march_update<FAST>(kappa, F, u0, a.alpha, a.beta, a.gamma, eps, eps2, a.f.dk1);
        if (lane_valid) out[o] = u0 + d;
        acc += d * d;
        um = u0; u0 = up;
        if ((r + 1) % a.g.item_rows == 0 || !more) {   // (wave-uniform) the item ends: strips begin on item boundaries
          march_store_sum(ml, acc, a.partials + (size_t)(r / a.g.item_rows) * a.g.nwc + wc);
          acc = 0.0;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) V[q] += cur.E[q] - cur.L[q];
    if (more) cur = nxt;
  }
}

template <int C, bool FAST, int KIND>
__global__ __launch_bounds__(CVH_BLOCK) void loc_wave_kernel(const CvhLocArgs *tab, int nmem, int parity)
{
  loc_wave_body<C, FAST, KIND, true>(((loc_table)tab)[march_member((loc_table)tab, nmem, [](const CVH_CONSTANT CvhLocArgs &m) { return m.wave_first; })], parity);
}

template <int C, bool FAST, int KIND>
__global__ __launch_bounds__(CVH_BLOCK) void loc_wave_kernel_one(const CvhLocArgs a)
{
  loc_wave_body<C, FAST, KIND, false>(a, 0);
}

// ONE workgroup per member: thread t adds items t, t + 256, ... in that order, block_reduce's fixed tree adds the threads; thread 0 writes
// the member's state block and (TABLE) its mirror in the leader's state table
template <bool TABLE, class Rec>
__device__ __forceinline__ void loc_finalize_body(const Rec &a)
{
  __shared__ double sred[4];
  CvhLocState *st = a.st;
  if (st->run.stopped) return;
  double acc[1] = {0.0};
  for (int it = threadIdx.x; it < a.g.nitems; it += CVH_BLOCK) acc[0] += a.partials[it];
  const double total = block_reduce<1>(acc, sred);
  if (threadIdx.x != 0) return;
  const double nrm = sqrt(total);
  const int t = st->run.steps_done;   // index of the iteration just executed
  if (a.trace && t < a.trace_cap) a.trace[t] = nrm;
  const int stopped = nrm <= a.stop ? 1 : 0;   // after the update
  st->norm = nrm;
  st->run.steps_done = t + 1;
  if (stopped) st->run.stopped = 1;
  if (TABLE) {
    CvhLocState *mirror = a.st_mirror;
    mirror->norm = nrm;
    mirror->run.steps_done = t + 1;
    mirror->run.stopped = stopped;
  }
}

__global__ __launch_bounds__(CVH_BLOCK) void loc_finalize_kernel(const CvhLocArgs *tab) { loc_finalize_body<true>(((loc_table)tab)[blockIdx.x]); }
__global__ __launch_bounds__(CVH_BLOCK) void loc_finalize_kernel_one(const CvhLocArgs a) { loc_finalize_body<false>(a); }

template <int C>
hipError_t launch_wave(const CvhLocArgs *tab, int nmem, unsigned grid_, int parity, int fast, int kind, hipStream_t s, const CvhLocArgs *one)
{
  const dim3 grid(grid_), block(CVH_BLOCK);
  if (one) {
    if (kind == CVH_LOC_TSUM) hipLaunchKernelGGL((loc_wave_kernel_one<C, false, CVH_LOC_TSUM>), grid, block, 0, s, *one);
    else if (kind == CVH_LOC_MEANS) hipLaunchKernelGGL((loc_wave_kernel_one<C, false, CVH_LOC_MEANS>), grid, block, 0, s, *one);
    else if (fast) hipLaunchKernelGGL((loc_wave_kernel_one<C, true, CVH_LOC_STEP>), grid, block, 0, s, *one);
    else hipLaunchKernelGGL((loc_wave_kernel_one<C, false, CVH_LOC_STEP>), grid, block, 0, s, *one);
    return hipGetLastError();
  }
  if (kind == CVH_LOC_TSUM) hipLaunchKernelGGL((loc_wave_kernel<C, false, CVH_LOC_TSUM>), grid, block, 0, s, tab, nmem, parity);
  else if (kind == CVH_LOC_MEANS) hipLaunchKernelGGL((loc_wave_kernel<C, false, CVH_LOC_MEANS>), grid, block, 0, s, tab, nmem, parity);
  else if (fast) hipLaunchKernelGGL((loc_wave_kernel<C, true, CVH_LOC_STEP>), grid, block, 0, s, tab, nmem, parity);
  else hipLaunchKernelGGL((loc_wave_kernel<C, false, CVH_LOC_STEP>), grid, block, 0, s, tab, nmem, parity);
  return hipGetLastError();
}

template <int C>
hipError_t launch_rows(const CvhLocArgs *tab, int nmem, unsigned grid_, int parity, int fast, int pass, hipStream_t s, const CvhLocArgs *one)
{
  const dim3 grid(grid_), block(CVH_BLOCK);
  if (one) {
    if (pass == CVH_LOC_TSUM) hipLaunchKernelGGL((loc_row_kernel_one<C, 2, false>), grid, block, 0, s, *one);
    else if (pass == CVH_LOC_MEANS) {
      if (fast) hipLaunchKernelGGL((loc_row_kernel_one<C, 1, false>), grid, block, 0, s, *one);
      else hipLaunchKernelGGL((loc_row_kernel_one<C, 0, false>), grid, block, 0, s, *one);
    } else if (fast) hipLaunchKernelGGL((loc_row_kernel_one<C, 1, true>), grid, block, 0, s, *one);
    else hipLaunchKernelGGL((loc_row_kernel_one<C, 0, true>), grid, block, 0, s, *one);
    return hipGetLastError();
  }
  if (pass == CVH_LOC_TSUM) hipLaunchKernelGGL((loc_row_kernel<C, 2, false>), grid, block, 0, s, tab, nmem, parity);
  else if (pass == CVH_LOC_MEANS) {
    if (fast) hipLaunchKernelGGL((loc_row_kernel<C, 1, false>), grid, block, 0, s, tab, nmem, parity);
    else hipLaunchKernelGGL((loc_row_kernel<C, 0, false>), grid, block, 0, s, tab, nmem, parity);
  } else if (fast) hipLaunchKernelGGL((loc_row_kernel<C, 1, true>), grid, block, 0, s, tab, nmem, parity);
  else hipLaunchKernelGGL((loc_row_kernel<C, 0, true>), grid, block, 0, s, tab, nmem, parity);
  return hipGetLastError();
}

}  // namespace

// Items: cvh_march_rows rows each (the order of the norm's sum follows them).  A strip -- what one wave marches down -- is the smallest
// whole number of items with at least CVH_LOC_LEAD (2 R + 1) rows.
CvhLocGeom cvh_loc_geometry(int h, int w, int radius)
{
  CvhLocGeom g;
  g.nwc = (w + CVH_MARCH_COLS - 1) / CVH_MARCH_COLS;
  g.item_rows = cvh_march_rows(h, g.nwc);
  g.nitem_rows = (h + g.item_rows - 1) / g.item_rows;
  g.nitems = g.nitem_rows * g.nwc;
  const int lead = CVH_LOC_LEAD * (2 * radius + 1);
  const long long sr = (long long)g.item_rows * ((lead + g.item_rows - 1) / g.item_rows);
  g.strip_rows = (int)std::min(sr, (long long)g.item_rows * g.nitem_rows);   // (one strip holds the plane: no more items than there are)
  g.nstrips = (h + g.strip_rows - 1) / g.strip_rows;
  g.grid = (unsigned)(((long long)g.nstrips * g.nwc + CVH_BLOCK / 64 - 1) / (CVH_BLOCK / 64));
  g.nseg = (w + CVH_WINDOW_SEGMENT - 1) / CVH_WINDOW_SEGMENT;
  g.row_grid = (unsigned)h * (unsigned)g.nseg;
  return g;
}

hipError_t cvh_launch_loc_rows(const CvhLocArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, int pass, hipStream_t s, const CvhLocArgs *one)
{
  return channels == 1 ? launch_rows<1>(tab, nmem, grid, parity, fast, pass, s, one) : launch_rows<3>(tab, nmem, grid, parity, fast, pass, s, one);
}

hipError_t cvh_launch_loc_wave(const CvhLocArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, int kind, hipStream_t s, const CvhLocArgs *one)
{
  return channels == 1 ? launch_wave<1>(tab, nmem, grid, parity, fast, kind, s, one) : launch_wave<3>(tab, nmem, grid, parity, fast, kind, s, one);
}

hipError_t cvh_launch_loc_finalize(const CvhLocArgs *tab, int nmem, hipStream_t s, const CvhLocArgs *one)
{
  if (one) hipLaunchKernelGGL(loc_finalize_kernel_one, dim3(1), dim3(CVH_BLOCK), 0, s, *one);
  else hipLaunchKernelGGL(loc_finalize_kernel, dim3((unsigned)nmem), dim3(CVH_BLOCK), 0, s, tab);
  return hipGetLastError();
}
