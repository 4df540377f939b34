// csv_wave_kernel.hip — wave-streaming variant of the fused CSV step (gfx950, wave64).
//
// Same arithmetic as csv_kernels.hip; data flow chosen from measurements on MI355X
// (tools/dp_rate_probe.hip, profiles/): the step is FP64-VALU-bound, and a wave64 FP64
// instruction costs ~3.3 SIMD-cycles at 4 waves/SIMD but ~2.4 at 8.  So this variant spends
// almost no LDS and few registers to run 7-8 waves per SIMD, and removes every VALU
// instruction that only moved data:
//   * each WAVE owns a strip of 63 output columns (lane 0 is the left halo column; lanes
//     1..63 produce pixels) and marches down `strip_rows` rows on its own: no workgroup
//     barrier inside the loop, waves drift apart and hide each other's memory latency;
//   * u(i-1), u(i), u(i+1) of the lane's own column and the previous row's normalised
//     y-gradient live in registers; rows are loaded straight into registers 4 rows ahead
//     (coalesced 512-byte wave loads), the image 4 rows ahead;
//   * x-neighbours go through a 4-slot, 66-double per-wave LDS row buffer (written when a
//     row arrives, read one row ahead of use: no exposed LDS latency, no VALU);
//     the two extra halo columns of 4 rows are fetched by 8 lanes in one load;
//   * the left neighbour's normalised x-gradient comes by DPP from lane-1; lane 0 computes
//     the halo column's gradient like any other lane, so nothing is recomputed per tile;
//   * borders: clamped column/row indices are BORDER_REPLICATE on u; the second-level rule
//     (kappa_x(.,0) = 0, kappa_y(0,.) = 0, src/main.cpp:371-372) is a 0/1 factor.
// One partial row of sums per workgroup; finalisation as in the other variants.
#include "csv_device.h"
#include "buffer_ops.h"
#include "wave_math.h"
#include "chain_device.h"
#include <type_traits>

using namespace cvh_dev;

namespace {

constexpr int WCOLS = 63;   // output columns per wave
constexpr int XPITCH = 66;  // exchange row: [0] = col-2 of lane 0, [1..64] = lanes, [65] = col+1 of lane 63
constexpr int IMGP = 80;     // bytes per row of the per-wave image tile (5 x 16-byte pieces)

template <int C, bool FAST, bool LUT, int G>
struct WaveSmem {
  static constexpr int R = 4 * G;                                          // rows per group = ring slots
  static constexpr int NS = cvh_nsums(C);
  static constexpr int off_x = 0;                                          // 4 waves x XSLOTS x XPITCH
  static constexpr int wave_doubles = R * XPITCH + 64 + C * R * IMGP / 8;  // row slots + scratch + image tile
  static constexpr int off_red = off_x + 4 * wave_doubles;                 // 4*NS
  static constexpr int off_fin = off_red + 4 * NS + (4 * NS) % 2;          // NS
  static constexpr int off_atan = off_fin + NS + NS % 2;                   // FAST: CVH_ATAN2_N
  static constexpr int off_lut = (off_atan + (FAST ? CVH_ATAN2_N + 1 : 0) + 1) & ~1;  // LUT: C*256 x {term, I}, 16-byte aligned
  static constexpr int off_flag = off_lut + (LUT ? C * 512 : 0);
  static constexpr int doubles = off_flag + 2;
  static constexpr size_t bytes = (size_t)doubles * sizeof(double);
};

// POL: cache policy of the level-set stores (1 = sc1 write-through while the pair fits the Infinity Cache: 1000^2 12.4 -> 11.65 us; beyond
// it write-through costs -- 6144^2: 144 -> 171 us; wave2_device.h has the 2-pixel kernel's figures), chosen by the host (wave_pol)
// Two entry points share one body (csv_wave_body.inc), textually, so that the context's own kernel compiles to exactly the ISA it
// had before the batch entry point existed (an always-inline __device__ body is simplified before it is inlined, and the
// result differs).  In the body, `a` is the context's launch arguments and `blk` the workgroup's index in the context's own grid.
template <int C, bool FAST, bool LUT, int MINW, bool IMGV, int G, int POL = 0>
__global__ __launch_bounds__(CVH_BLOCK, MINW) void csv_wave_kernel(const CvhStepArgs a)
{
  const unsigned blk = blockIdx.x;
#include "csv_wave_body.inc"
}

// Fused batch entry point (cvh_internal.h, CvhBatchArgs): the same body for the member this workgroup belongs to, with the
// member-local workgroup index; the member's arguments are read through the scalar cache
template <int C, bool FAST, bool LUT, int MINW, bool IMGV, int G, int POL = 0>
__global__ __launch_bounds__(CVH_BLOCK, MINW) void csv_wave_batch_kernel(const CvhBatchArgs b)
{
  unsigned blk;
  const CvhStepArgs *const ap = batch_member(b, &blk);
  if (!ap) return;   // padding of the member's section
  const CvhStepArgs &a = *ap;
#include "csv_wave_body.inc"
}

template <int C, bool FAST, bool LUT, int MINW, int G>
hipError_t launch_wave_g(const CvhStepArgs &a, hipStream_t s, const CvhBatchLaunch *batch)
{
  using L = WaveSmem<C, FAST, LUT, G>;
  static_assert(L::bytes <= 64 * 1024, "dynamic LDS above 64 KiB would need hipFuncSetAttribute");
  // Ask for 1/W of the CU's 160 KiB of LDS: the hardware can then place at most W workgroups on
  // a CU, so a grid of <= W x CUs workgroups spreads evenly instead of packing some CUs fuller
  // than others (the step is VALU-bound: the fullest CU sets the kernel time).
  size_t lds = L::bytes;
  if (a.wave_lds_cap) {
    size_t cap = ((size_t)160 * 1024 / (size_t)(a.wave_minw > 2 ? a.wave_minw : 3)) & ~(size_t)511;
    if (cap > 64 * 1024) cap = 64 * 1024;
    if (cap > lds) lds = cap;
  }
  const bool imgv = a.w % 16 == 0 && a.w >= 80 && a.wave_imgv;
  const int extra = (FAST && a.chain) ? 1 : 0;   // the bookkeeping workgroup of chain mode
  if constexpr (FAST && LUT && G == 1) {   // the shipped flavours exist with write-through stores too
    if (a.wave_pol == 1) {
      if (imgv) CVH_LAUNCH_B((csv_wave_kernel<C, FAST, LUT, MINW, true, G, 1>), (csv_wave_batch_kernel<C, FAST, LUT, MINW, true, G, 1>), a.nparts + extra, lds, s, a, batch, "csv_wave_kernel<%d, %s, %s, %d, true, %d, 1>", C, CVH_TF(FAST), CVH_TF(LUT), MINW, G);
      else CVH_LAUNCH_B((csv_wave_kernel<C, FAST, LUT, MINW, false, G, 1>), (csv_wave_batch_kernel<C, FAST, LUT, MINW, false, G, 1>), a.nparts + extra, lds, s, a, batch, "csv_wave_kernel<%d, %s, %s, %d, false, %d, 1>", C, CVH_TF(FAST), CVH_TF(LUT), MINW, G);
      return hipGetLastError();
    }
  }
  if (imgv) CVH_LAUNCH_B((csv_wave_kernel<C, FAST, LUT, MINW, true, G>), (csv_wave_batch_kernel<C, FAST, LUT, MINW, true, G>), a.nparts + extra, lds, s, a, batch, "csv_wave_kernel<%d, %s, %s, %d, true, %d, 0>", C, CVH_TF(FAST), CVH_TF(LUT), MINW, G);
  else CVH_LAUNCH_B((csv_wave_kernel<C, FAST, LUT, MINW, false, G>), (csv_wave_batch_kernel<C, FAST, LUT, MINW, false, G>), a.nparts + extra, lds, s, a, batch, "csv_wave_kernel<%d, %s, %s, %d, false, %d, 0>", C, CVH_TF(FAST), CVH_TF(LUT), MINW, G);
  return hipGetLastError();
}

template <int C, bool FAST, bool LUT, int MINW>
hipError_t launch_wave_v(const CvhStepArgs &a, hipStream_t s, const CvhBatchLaunch *batch)
{
  // 8-row groups (wave_depth 8) double the time a request has to land; built where registers allow
  if constexpr (C == 1 && FAST && LUT) { if (a.wave_depth >= 8) return launch_wave_g<C, FAST, LUT, MINW, 2>(a, s, batch); }
  return launch_wave_g<C, FAST, LUT, MINW, 1>(a, s, batch);
}

template <int C>
hipError_t launch_wave_c(const CvhStepArgs &a, int fast, hipStream_t s, const CvhBatchLaunch *batch)
{
  if (!fast) return launch_wave_v<C, false, false, (C == 1 ? 3 : 2)>(a, s, batch);
  if constexpr (C == 3) {  // 9 accumulators, 3 image tiles: fits 168 registers (3 waves/SIMD) without spilling
    return a.use_lut ? launch_wave_v<C, true, true, 3>(a, s, batch) : launch_wave_v<C, true, false, 3>(a, s, batch);
  } else {
    // 5 waves/SIMD (96 registers) is the most this kernel reaches without spilling; 4 is kept for comparison
    if (a.wave_minw >= 5) return a.use_lut ? launch_wave_v<C, true, true, 5>(a, s, batch) : launch_wave_v<C, true, false, 4>(a, s, batch);
    return a.use_lut ? launch_wave_v<C, true, true, 4>(a, s, batch) : launch_wave_v<C, true, false, 4>(a, s, batch);
  }
}

}  // namespace

int cvh_wave_cols() { return WCOLS; }

hipError_t cvh_launch_wave(const CvhStepArgs &a, int channels, int fast, hipStream_t s, const CvhBatchLaunch *batch)
{
  return channels == 1 ? launch_wave_c<1>(a, fast, s, batch) : launch_wave_c<3>(a, fast, s, batch);
}
