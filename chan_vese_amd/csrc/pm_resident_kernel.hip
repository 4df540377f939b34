// pm_resident_kernel.hip — Perona-Malik (src/main.cpp:478-560) on a cache-resident plane (gfx950, wave64): the FP64 state of one
// channel lives in LDS for a whole chunk of time steps.
//
// A 2048^2 plane is 32 MiB of doubles; the 256 CUs of an MI355X hold 40 MiB of LDS.  One cooperative launch cuts the plane into
// tiles_y x tiles_x tiles of <= 128 rows x 128 columns, ONE workgroup (8 waves) per tile and per CU, loads every tile with a halo
// ring of width 2 into its CU's LDS once, runs `res_steps` time steps on it and writes the tiles back at the end.  A launch per
// step (or per two steps, pm_wave_k2_kernel.hip) moves the plane through the memory system every step; here a step moves the
// tiles' borders only, and -- unlike the CSV iteration (csv_resident_kernel.hip) -- a Perona-Malik step has no global sum, so
// there is NO grid barrier: a tile waits for its up-to-eight neighbours only.
//
// One step of a tile:
//   1. (steps > 0) every thread polls its <= 3 cells of the halo ring in the neighbours' border pieces until they carry the previous
//      step: an entry of the border buffer is 16 bytes {value, tag = (launch serial, step)}, written with ONE store, so there is no
//      separate signal to wait for (one memory round trip instead of signal-then-data); at the image's border the cell is the
//      clamped pixel (BORDER_REPLICATE), own tile or a neighbour's;
//   2. every wave computes its band of NR rows x 128 columns (lane <-> two adjacent columns) from the OLD tile: the row pass of the
//      Sobel pair (:503-504) is shared by the three rows of g that need it, g = 1 / (1 + |Sobel|^2 / K^2) (:503-520) of the own
//      columns marches down in registers, its x-neighbours come over DPP, the two edge columns' g (tile columns -1 and TW) from a
//      per-wave pre-pass; a row is rewritten in place as soon as it is computed, except the band's first and last two rows (the
//      neighbouring bands still read them), which wait in registers for
//   3. the workgroup barrier;
//   4. the tile's border -- top / bottom two rows, left / right two columns: a step reaches two pixels (g of a neighbour needs
//      the neighbour's 3 x 3) -- goes into a double-buffered global buffer with agent-scope 16-byte stores: from the registers while
//      the band is computed (full tiles), from LDS behind the barrier (ragged tiles).
// Every wait is a bounded poll: a thread that gives up raises CvhResident::error and its workgroup leaves, and so does everybody
// waiting for it -- the grid always drains; the host reports the error.
//
// The arithmetic of a pixel is pm_wave_k2_kernel.hip's (hence pm_wave_kernel's) operation by operation in both flavours: STRICT
// stays bit-exact against the oracle, FAST gives the very doubles the per-launch kernels give.
#include "csv_device.h"
#include "buffer_ops.h"
#include "wave_math.h"

using namespace cvh_dev;

namespace {

constexpr int PT_W = 128;                 // tile width: 64 lanes x 2 pixels
constexpr int PT_HMAX = 128;              // most rows a tile may have (LDS)
constexpr int PT_PITCH = PT_W + 4;        // doubles per LDS row: tile columns -2 .. 129
constexpr int PT_WAVES = 8, PT_THREADS = 64 * PT_WAVES;
constexpr int PT_HALO = 8 * PT_W;         // doubles a tile publishes per step: rows 0, 1, TH-2, TH-1, columns 0, 1, TW-2, TW-1
constexpr int PT_RING = 4 * PT_PITCH + 4 * PT_HMAX;          // cells of the halo ring (rows -2, -1, TH, TH+1; columns -2, -1, TW, TW+1)
constexpr int PT_GATHER = (PT_RING + PT_THREADS - 1) / PT_THREADS;   // ring cells per thread

constexpr int kRowsPerSched = 2;          // a scheduling barrier behind every second row of the march (round 3, pm_sched_variants.txt: 1, 4 or no barrier: no faster, more registers)

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4s_t __attribute__((ext_vector_type(4)));

struct PmResSmem {
  static constexpr int off_I = 0;                                          // (PT_HMAX + 4) rows x PT_PITCH: tile rows -2 .. TH+1
  static constexpr int off_edge = off_I + (PT_HMAX + 4) * PT_PITCH;       // per wave: g of tile column -1 [16], of tile column TW [16]
  static constexpr int off_flag = off_edge + PT_WAVES * 32;
  static constexpr int off_stage = off_flag + 2;                          // per wave: the four edge columns of up to four rows [4][4], on their way to the border buffer
  static constexpr int off_rstage = off_stage + PT_WAVES * 16;             // per wave: one row of the tile [PT_W] on its way to the border buffer (waves 0 and 7 of a full tile)
  static constexpr int doubles = off_rstage + PT_WAVES * PT_W;
  static constexpr size_t bytes = (size_t)doubles * sizeof(double);
};
static_assert(PmResSmem::bytes <= 160 * 1024, "the tile with its halo ring must fit one CU's LDS");

__device__ __forceinline__ unsigned ld_agent(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 16-byte agent-scope (sc1) accesses to the border buffer: one entry {value, tag}, one transaction
__device__ __forceinline__ u32x4s_t ld_line16(const void *base, unsigned byte_off)
{
  return __builtin_amdgcn_raw_buffer_load_b128(make_rsrc(base, 0x7fffffffu), byte_off, 0u, 16 /* sc1 */);
}
__device__ __forceinline__ u32x4s_t tagged(double v, unsigned tag_lo, unsigned tag_hi)
{
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return u32x4s_t{(unsigned)b, (unsigned)(b >> 32), tag_lo, tag_hi};
}

// lane l gets lane l + 1's v (wave_shl:1); lane 63 has no source lane and keeps `old` (wave_math.h has the other direction)
__device__ __forceinline__ double dpp_from_right_or(double old, double v)
{
  const long long vb = __double_as_longlong(v), ob = __double_as_longlong(old);
  const int lo = __builtin_amdgcn_update_dpp((int)ob, (int)vb, 0x130 /*wave_shl:1*/, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(ob >> 32), (int)(vb >> 32), 0x130, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <bool FAST, int NR>
__global__ __launch_bounds__(PT_THREADS, 1) void pm_resident_kernel(const CvhPmArgs a)
{
  const int bid = (int)blockIdx.x;          // the launch is one plane: its tiles are the launch's
  constexpr int tbase = 0;
  const int ntiles = a.tiles_y * a.tiles_x;
#include "pm_resident_body.inc"
}

// Batch entry point (cvh_perona_malik_batch, api.hip; CvhPmBatchArgs, cvh_internal.h): the planes of several contexts share one cooperative
// launch.  map[blockIdx.x] names the workgroup's plane; the plane's tiles are a contiguous run of the grid starting at its tile_base, and
// its arguments (read through the scalar cache) are what the plane's own launch would be given.  A step has no global sum, so a tile
// waits for its own plane's neighbours only, and a plane's tiles leave after the plane's own res_steps.
template <bool FAST, int NR>
__global__ __launch_bounds__(PT_THREADS, 1) void pm_resident_batch_kernel(const CvhPmBatchArgs b)
{
  typedef const __attribute__((address_space(4))) unsigned *const_u32_p;
  typedef const __attribute__((address_space(4))) CvhPmBatchPlane *const_plane_p;
  const unsigned p = ((const_u32_p)b.map)[blockIdx.x];
  const CvhPmBatchPlane *const pl = (const CvhPmBatchPlane *)((const_plane_p)b.planes + p);
  const CvhPmArgs a = pl->a;
  const int tbase = pl->tile_base;
  const int bid = (int)blockIdx.x - tbase;
  const int ntiles = b.ntiles;
#include "pm_resident_body.inc"
}

}  // namespace

size_t cvh_pm_resident_lds_bytes() { return PmResSmem::bytes; }
int cvh_pm_resident_halo_doubles() { return 2 * PT_HALO; }   // 16-byte entries {value, tag}

namespace {
typedef void (*PmResKernel)(const CvhPmArgs);
PmResKernel pm_res_kernel(int fast, int nr)
{
  switch (nr) {
    case 2: return fast ? pm_resident_kernel<true, 2> : pm_resident_kernel<false, 2>;
    case 4: return fast ? pm_resident_kernel<true, 4> : pm_resident_kernel<false, 4>;
    case 8: return fast ? pm_resident_kernel<true, 8> : pm_resident_kernel<false, 8>;
    case 16: return fast ? pm_resident_kernel<true, 16> : pm_resident_kernel<false, 16>;
  }
  return nullptr;
}
}  // namespace

// Workgroups of the resident kernel one CU holds (0: not launchable): the least over the instantiations.
int cvh_pm_resident_blocks_per_cu()
{
  static int cached = -1;
  if (cached >= 0) return cached;
  int least = 1 << 30;
  for (int fast = 0; fast < 2; ++fast)
    for (int nr = 2; nr <= 16; nr *= 2) {
      const void *k = reinterpret_cast<const void *>(pm_res_kernel(fast, nr));
      int n = 0;
      if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PmResSmem::bytes) != hipSuccess ||
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, PT_THREADS, PmResSmem::bytes) != hipSuccess) {
        (void)hipGetLastError();
        return cached = 0;
      }
      if (n < least) least = n;
    }
  return cached = least;
}

namespace {
typedef void (*PmResBatchKernel)(const CvhPmBatchArgs);
PmResBatchKernel pm_res_batch_kernel(int fast, int nr)
{
  switch (nr) {
    case 2: return fast ? pm_resident_batch_kernel<true, 2> : pm_resident_batch_kernel<false, 2>;
    case 4: return fast ? pm_resident_batch_kernel<true, 4> : pm_resident_batch_kernel<false, 4>;
    case 8: return fast ? pm_resident_batch_kernel<true, 8> : pm_resident_batch_kernel<false, 8>;
    case 16: return fast ? pm_resident_batch_kernel<true, 16> : pm_resident_batch_kernel<false, 16>;
  }
  return nullptr;
}
}  // namespace

// The same for the batch entry points (they must hold one workgroup per CU as well).
int cvh_pm_resident_batch_blocks_per_cu()
{
  static int cached = -1;
  if (cached >= 0) return cached;
  int least = 1 << 30;
  for (int fast = 0; fast < 2; ++fast)
    for (int nr = 2; nr <= 16; nr *= 2) {
      const void *k = reinterpret_cast<const void *>(pm_res_batch_kernel(fast, nr));
      int n = 0;
      if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PmResSmem::bytes) != hipSuccess ||
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, PT_THREADS, PmResSmem::bytes) != hipSuccess) {
        (void)hipGetLastError();
        return cached = 0;
      }
      if (n < least) least = n;
    }
  return cached = least;
}

hipError_t cvh_launch_pm_resident(const CvhPmArgs &a, hipStream_t s)
{
  const PmResKernel kern = pm_res_kernel(a.fast, a.res_band_rows);
  if (!kern) return hipErrorInvalidValue;
  if (a.note) {
    cvh_fill_note(a.note, (unsigned)(a.tiles_x * a.tiles_y), PT_THREADS, PmResSmem::bytes, "pm_resident_kernel<%s, %d>", a.fast ? "true" : "false", a.res_band_rows);
    return hipSuccess;
  }
  CvhPmArgs copy = a;
  void *params[] = {&copy};
  return hipLaunchCooperativeKernel(reinterpret_cast<const void *>(kern), dim3(a.tiles_x * a.tiles_y), dim3(PT_THREADS), params, (unsigned)PmResSmem::bytes, s);
}

// grid = b.ntiles workgroups; every instantiation's LDS attribute was set by cvh_pm_resident_batch_blocks_per_cu (the host asks it first)
hipError_t cvh_launch_pm_resident_batch(const CvhPmBatchArgs &b, int fast, int nr, hipStream_t s, CvhLaunchNote *note)
{
  const PmResBatchKernel kern = pm_res_batch_kernel(fast, nr);
  if (!kern || b.ntiles < 1 || b.ntiles > CVH_RESIDENT_MAX_TILES) return hipErrorInvalidValue;
  if (note) {
    cvh_fill_note(note, (unsigned)b.ntiles, PT_THREADS, PmResSmem::bytes, "pm_resident_batch_kernel<%s, %d>", fast ? "true" : "false", nr);
    return hipSuccess;
  }
  CvhPmBatchArgs copy = b;
  void *params[] = {&copy};
  return hipLaunchCooperativeKernel(reinterpret_cast<const void *>(kern), dim3(b.ntiles), dim3(PT_THREADS), params, (unsigned)PmResSmem::bytes, s);
}
