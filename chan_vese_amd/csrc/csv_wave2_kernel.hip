// csv_wave2_kernel.hip — wave-streaming CSV step with TWO pixels per lane (gfx950, wave64, 1 channel).
//
// Same arithmetic and the same data flow as csv_wave_kernel.hip (buffer loads/stores with dropped
// lanes, next group parked in a per-wave LDS ring, branch-free interior groups), but a lane owns two
// ADJACENT columns: a wave covers 128 columns (lane 0 holds the two west halo columns, lanes 1..63
// produce 126 pixels per row).  Measured on MI355X: one vector-memory INSTRUCTION per
// wave-row costs about as much whatever it moves, so 16-byte row loads/stores halve that cost per
// pixel; the LDS exchange and the DPP move of the west neighbour's normalised gradient are halved
// as well (one of the two x-neighbours of a pixel is in the same lane), the east halo is one column,
// and the two pixels of a lane are independent dependency chains.
//   ring slot (130 doubles): [a0 b0 a1 b1 ... a63 b63 | east extra]; per-lane read addresses implement
//   the BORDER_REPLICATE clamps at the image's left / right edges, so the row values need no selects.
// Workgroup = 2 wave-columns x 2 strips (a 4096-wide image has 33 wave-columns: pairs waste less than
// quads).  Requires w % 16 == 0 and w >= 144 (16-byte image pieces); other shapes use kernel 2.
// C = 3 (round 3, FAST only): one image tile per channel (two piece loads per group), the samples are read from the
// tile inside the row (no per-group sample registers), and the region term sum_k [l2k (I_k - c2k)^2 - l1k (I_k - c1k)^2] beta
// + gamma is three table lookups.  (The table-free quadratic form sum_k (qa_k I_k + qb_k) I_k + qc of round 3 -- 81 against 72 us --
// lives in tools/experiments/pruned_flavours/.)
#include "csv_device.h"
#include "buffer_ops.h"
#include "wave_math.h"
#include "chain_device.h"
#include "wave2_device.h"
#include <type_traits>

using namespace cvh_dev;

namespace {

// Two entry points share one body (csv_wave2_body.inc), textually, so that the context's own kernel compiles to exactly the ISA it
// had before the batch entry point existed (an always-inline __device__ body is simplified before it is inlined, and the
// result differs).  In the body, `a` is the context's launch arguments and `blk` the workgroup's index in the context's own grid.
template <int C, bool FAST, int MINW, int POL, bool ST32>
__global__ __launch_bounds__(CVH_BLOCK, MINW) void csv_wave2_kernel(const CvhStepArgs a)
{
  constexpr bool OB = false;
  const unsigned blk = blockIdx.x;
#include "csv_wave2_body.inc"
}

// Fused batch entry point (cvh_internal.h, CvhBatchArgs): the same body for the member this workgroup belongs to, with the
// member-local workgroup index; the member's arguments are read through the scalar cache
template <int C, bool FAST, int MINW, int POL, bool ST32>
__global__ __launch_bounds__(CVH_BLOCK, MINW) void csv_wave2_batch_kernel(const CvhBatchArgs b)
{
  unsigned blk;
  const CvhStepArgs *const ap = batch_member(b, &blk);
  if (!ap) return;   // padding of the member's section
  const CvhStepArgs &a = *ap;
  constexpr bool OB = false;
#include "csv_wave2_body.inc"
}

// One-buffer flow (one channel, FAST, FP64 state; no batch entry point): the same body with OB = true updates the level set in place in the
// padded slab of cvh_internal.h (cvh_ob_*).  What a wave reads of cells that ANOTHER wave writes -- lane 0's halo pair, the east extra, the
// rows s0 - 2, s0 - 1 and s1 around its strip -- comes from the row pads and the shadow rows of the launch's read parity, which their owners
// wrote one iteration earlier; every wave writes the other parity beside its rows.  Its own rows it has loaded before it stores them.
template <int POL>
__global__ __launch_bounds__(CVH_BLOCK, 3) void csv_wave2_ob_kernel(const CvhStepArgs a)
{
  constexpr int C = 1, MINW = 3;
  constexpr bool FAST = true, ST32 = false, OB = true;
  const unsigned blk = blockIdx.x;
#include "csv_wave2_body.inc"
}

// dense plane -> slab: workgroup r < h copies row r and fills its pad of parity `par`; workgroup h + q fills shadow row q of that parity
__global__ __launch_bounds__(CVH_BLOCK) void ob_pack_kernel(const double *dense, double *slab, const int *tab, int h, int w, int nwc, int nstrips, int par)
{
  const int pitch = cvh_ob_pitch(w, nwc), r = (int)blockIdx.x;
  if (r < h) {
    const double *src = dense + (size_t)r * w;
    double *dst = slab + (size_t)r * pitch;
    for (int j = threadIdx.x; j < w; j += CVH_BLOCK) dst[j] = src[j];
    for (int q = threadIdx.x; q < 4 * nwc; q += CVH_BLOCK) {
      const int wc = q >> 2, b = (q >> 1) & 1, col = W2 * wc + (b ? 0 : W2 - 2) + (q & 1);
      dst[cvh_ob_slot(w, nwc, par, wc, b) + (q & 1)] = col < w ? src[col] : 0.0;
    }
    return;
  }
  const int q = r - h, from = tab[(q / 3) * CVH_OB_TAB + 5 + q % 3];
  if (from < 0) return;
  const double *src = dense + (size_t)from * w;
  double *dst = slab + (size_t)cvh_ob_shadow_row(h, nstrips, par, q) * pitch;
  for (int j = threadIdx.x; j < w; j += CVH_BLOCK) dst[j] = src[j];
}

__global__ __launch_bounds__(CVH_BLOCK) void ob_unpack_kernel(const double *slab, double *dense, int w, int pitch)
{
  const double *src = slab + (size_t)blockIdx.x * pitch;
  double *dst = dense + (size_t)blockIdx.x * w;
  for (int j = threadIdx.x; j < w; j += CVH_BLOCK) dst[j] = src[j];
}

template <int C, bool FAST, int MINW, int POL, bool ST32 = false>
hipError_t launch_wave2(const CvhStepArgs &a, hipStream_t s, const CvhBatchLaunch *batch)
{
  using L = Wave2Smem<FAST, C>;
  static_assert(L::bytes <= 64 * 1024, "dynamic LDS above 64 KiB would need hipFuncSetAttribute");
  static_assert(MINW * L::bytes <= 160 * 1024, "the kernel is compiled for MINW workgroups per CU: their LDS must fit the CU's 160 KiB");
  const int extra = (FAST && a.chain) ? 1 : 0;   // the bookkeeping workgroup
  CVH_LAUNCH_B((csv_wave2_kernel<C, FAST, MINW, POL, ST32>), (csv_wave2_batch_kernel<C, FAST, MINW, POL, ST32>), a.nparts + extra, L::bytes, s, a, batch,
               "csv_wave2_kernel<%d, %s, %d, %d, %s>", C, CVH_TF(FAST), MINW, POL, CVH_TF(ST32));
  return hipGetLastError();
}

template <int POL>
hipError_t launch_wave2_ob(const CvhStepArgs &a, hipStream_t s)
{
  using L = Wave2Smem<true, 1>;
  CVH_LAUNCH((csv_wave2_ob_kernel<POL>), a.nparts + (a.chain ? 1 : 0), L::bytes, s, a, "csv_wave2_ob_kernel<%d>", POL);
  return hipGetLastError();
}

}  // namespace

int cvh_wave2_cols() { return W2; }

hipError_t cvh_launch_ob_pack(const double *dense, double *slab, const int *tab, int h, int w, int nwc, int nstrips, int par, hipStream_t s)
{
  hipLaunchKernelGGL(ob_pack_kernel, dim3(h + 3 * nstrips), dim3(CVH_BLOCK), 0, s, dense, slab, tab, h, w, nwc, nstrips, par);
  return hipGetLastError();
}

hipError_t cvh_launch_ob_unpack(const double *slab, double *dense, int h, int w, int nwc, hipStream_t s)
{
  hipLaunchKernelGGL(ob_unpack_kernel, dim3(h), dim3(CVH_BLOCK), 0, s, slab, dense, w, cvh_ob_pitch(w, nwc));
  return hipGetLastError();
}

// Instantiations <channels, FAST, waves per SIMD, cache policy of the rows, FP32 state>: <1, false, 2, 1, false> STRICT; <1 | 3, true, 3,
// POL, false> FAST (wave2_device.h: POL 1 write-through stores + sc0 loads, 0 plain, 2 plain stores + non-temporal loads -- diagnostic);
// <1 | 3, true, 3, POL, true> the DECLARED FP32-state mode (option "state" = 32).  Round 3 also shipped a 4-waves/SIMD flavour (95.7
// against 57.3 us at 4096^2) and a table-free 3-channel region term (81 against 72 us): neither was ever chosen, neither is a fallback --
// tools/experiments/pruned_flavours/README.md.
hipError_t cvh_launch_wave2(const CvhStepArgs &a, int channels, int fast, hipStream_t s, const CvhBatchLaunch *batch)
{
  if (a.state32) {   // FAST only (api.hip refuses the combination with STRICT)
    if (channels == 3) return a.wave_pol ? launch_wave2<3, true, 3, 1, true>(a, s, batch) : launch_wave2<3, true, 3, 0, true>(a, s, batch);
    return a.wave_pol ? launch_wave2<1, true, 3, 1, true>(a, s, batch) : launch_wave2<1, true, 3, 0, true>(a, s, batch);
  }
  if (channels == 3) return a.wave_pol ? launch_wave2<3, true, 3, 1>(a, s, batch) : launch_wave2<3, true, 3, 0>(a, s, batch);   // FAST only (api.hip routes STRICT to kernel 2)
  if (!fast) return launch_wave2<1, false, 2, 1>(a, s, batch);
  if (a.one_buffer) {   // csv_run.hip selects it for a context's own launches only, with "wave_pol" 0 or 1
    if (batch || a.wave_pol == 2) return hipErrorInvalidValue;
    return a.wave_pol ? launch_wave2_ob<1>(a, s) : launch_wave2_ob<0>(a, s);
  }
  if (a.wave_pol == 2) return launch_wave2<1, true, 3, 2>(a, s, batch);
  return a.wave_pol ? launch_wave2<1, true, 3, 1>(a, s, batch) : launch_wave2<1, true, 3, 0>(a, s, batch);
}
