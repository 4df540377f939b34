// csv_resident_kernel.hip — cache-resident planes (gfx950, wave64, 1 or 3 channels, FAST arithmetic, chain-mode sums): the level set
// lives in LDS for a whole chunk of iterations.
//
// A 2048^2 level set is 32 MiB; the 256 CUs of an MI355X hold 40 MiB of LDS.  One cooperative launch cuts the plane into
// tiles_y x tiles_x tiles of <= 128 rows x 128 columns, ONE workgroup (8 waves) per tile and per CU, loads every tile into its
// CU's LDS once, runs `res_steps` iterations of src/main.cpp:963-1001 on it in place, and writes the tiles back at the end.
// What a launch per iteration pays every iteration -- the launch gap, the dispatch ramp, 7 rows of loads per 21-row strip before
// the first row computes, the drain of the last waves, every level-set byte through the memory system twice -- is paid once per
// chunk; what crosses workgroups per iteration is
//   * the tile's border rows / columns (the 7-point cross reaches 2 up / left, 1 down / right: 6 x 128 doubles per tile), through a
//     double-buffered global halo buffer, written and read with sc1 (agent scope), two doubles per 16-byte store / load;
//   * ONE grid barrier with a master.  A tile ARRIVES with three 16-byte agent-scope stores into its own 64-byte line {generation, sum
//     u_diff^2} {generation, sum H'} {generation, sum I H'} -- the last two as chain mode's fixed-point integers (chain_device.h) -- right
//     behind its reduction, before its border stores (those get their own signal line: only the neighbours wait for them).  Workgroup
//     0 is the master: four of its waves watch 64 arrival lines each without workgroup barriers (the other four do the tile's own border
//     work meanwhile), wave 0 adds the integers (exact, order-free: the totals the per-launch path's atomic adds produce), books the
//     iteration (norm, stop rule src/main.cpp:1000, trace row) and RELEASES everybody with one line per XCD that carries the leave bit and
//     the region means of the new level set.  The stop rule therefore fires at the reference's iteration with no extra iteration computed,
//     and no atomic is issued inside the launch.  (What the barrier costs and how it got here: DESIGN.md 4.1b.)
// Every wait is a bounded poll: a workgroup that gives up raises CvhResident::error and leaves, and so does everybody waiting
// for it -- the grid always drains; the host reports the error at the next synchronisation.
//
// Inside a tile: wave v owns a band of rows and all 128 columns (lane l <-> columns 2l, 2l + 1), marches down its band with
// u(i-1), u(i) in registers and u(i+1) and the x-neighbours read from the LDS tile one row ahead, and writes row i IN PLACE once it
// is computed.  Bands only meet at their first / last rows: every wave reads the two rows above its band and the row below it
// into registers before any wave writes (one workgroup barrier).  Column -1's normalised x-gradient, which lane 0 needs for
// kappa_x of column 0 and no lane owns, is computed for all rows of the tile by one thread per row before the march.
// The arithmetic of a pixel is csv_wave2_kernel.hip's FAST flavour operation by operation.
//
// Three channels (csv_resident_kernel<3, NRT>, option "resident" = 1): the same kernel along its template parameter C.  A tile holds three
// image tiles and three region-term tables in LDS beside the level set, so it has at most 96 rows (ResSmem<3>: 154 of 160 KiB); the
// arithmetic of a pixel is csv_wave2_kernel<3, ...>'s (pixel3: the region term summed over the channels' tables).  A tile arrives with FIVE
// pieces {sum u_diff^2} {sum H'} {sum I_k H'} k = 0..2, and the release is SIX pieces {generation, leave, c1_k} {generation, leave, c2_k} on a
// 128-byte line.  The pieces the one-channel kernel does not have live BEHIND everything it addresses in CvhResident (flag_c3, go_c3): the
// one-channel instantiations are instruction for instruction what they were before C existed.
#include "csv_device.h"
#include "buffer_ops.h"
#include "wave_math.h"
#include "chain_device.h"
#include <type_traits>

using namespace cvh_dev;

namespace {

constexpr int RT_W = 128;                 // tile width: 64 lanes x 2 pixels
constexpr int rt_hmax(int C) { return C == 1 ? 128 : 96; }   // most rows a tile may have (LDS: three channels keep three image tiles and three tables)
constexpr int RT_PITCH = 132;             // doubles per LDS row: tile columns -2 .. 129
// Poll cadences and waves per workgroup were A/B build macros in round 3 (profiles/r03_C4/resident_poll_variants.txt: s_sleep 1 between the
// master's polls and 3 between a workgroup's polls of its release line are a local optimum; 12 / 16 waves per workgroup: 17.4 / 33 us).
constexpr int kMasterSleep = 1, kReleaseSleep = 3;
constexpr int RT_WAVES = 8, RT_THREADS = 64 * RT_WAVES;
constexpr int RT_HALO = 6 * RT_W;         // doubles a tile publishes per iteration: bottom 2 rows, top row, right 2 columns, left column


typedef double double2_t __attribute__((ext_vector_type(2)));

template <int C>
struct ResSmem {
  static constexpr int NS = cvh_nsums(C);
  static constexpr int HMAX = rt_hmax(C);
  static constexpr int NP = 2 + C;                                          // sums a tile reports: sum u_diff^2, sum H', sum I_k H'
  static constexpr int NBC = 1 + 2 * C;                                     // broadcast doubles: the leave bit, c1_k, c2_k
  static constexpr int img_bytes = HMAX * RT_W;                             // one channel's image tile
  static constexpr int off_u = 0;                                           // (HMAX + 3) rows x RT_PITCH: tile rows -2 .. TH
  static constexpr int off_img = off_u + (HMAX + 3) * RT_PITCH;             // C x HMAX x 128 bytes
  static constexpr int off_lut = off_img + C * img_bytes / 8;               // C x 256 x {term, I}
  static constexpr int off_atan = off_lut + C * 512;                        // CVH_ATAN2_N (+1 pad)
  static constexpr int off_nxl = off_atan + CVH_ATAN2_N + 1;                // HMAX: normalised x-gradient of column -1
  static constexpr int off_red = off_nxl + HMAX;                            // RT_WAVES x NS
  static constexpr int off_flag = off_red + RT_WAVES * NS;
  static constexpr int doubles = off_flag + (NBC + 1) + (RT_WAVES + 1) / 2 + 1 + RT_WAVES / 2;   // NBC broadcast doubles, 12 ints, the master's RT_WAVES ints
  static constexpr size_t bytes = (size_t)doubles * sizeof(double);
  static_assert(RT_WAVES * NS >= NP * RT_WAVES + NP * (RT_WAVES / 2), "sred holds the tiles' 8 x NP partial sums and the master's 4 x NP");
  static_assert(bytes <= 160 * 1024, "the tile, its halo ring, the image tiles and the tables must fit one CU's LDS");
};
static_assert(64 * (RT_WAVES / 2) >= CVH_RESIDENT_MAX_TILES, "the master's four polling waves watch 64 arrival lines each");
static_assert(ResSmem<1>::bytes == 162328, "one channel: 128-row tiles, 159 of the CU's 160 KiB");
static_assert(ResSmem<3>::bytes == 157240, "three channels: 96-row tiles, 154 KiB (104 rows would need 165 KiB)");

__device__ __forceinline__ unsigned ld_agent(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(unsigned *p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_agent_f64(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent_f64(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 16-byte agent-scope (sc1) accesses to the synchronisation lines: one lane, one transaction.
typedef unsigned int u32x4r_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4r_t ld_line16(const void *base, unsigned byte_off)
{
  return __builtin_amdgcn_raw_buffer_load_b128(make_rsrc(base, 0x7fffffffu), byte_off, 0u, 16 /* sc1 */);
}
__device__ __forceinline__ void st_line16(void *base, unsigned byte_off, unsigned w0, unsigned w1, double d)
{
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  __builtin_amdgcn_raw_buffer_store_b128(u32x4r_t{w0, w1, (unsigned)b, (unsigned)(b >> 32)}, make_rsrc(base, 0x7fffffffu), byte_off, 0u, 16 /* sc1 */);
}
__device__ __forceinline__ void st_line16_u64(void *base, unsigned byte_off, unsigned w0, unsigned w1, unsigned long long b)
{
  __builtin_amdgcn_raw_buffer_store_b128(u32x4r_t{w0, w1, (unsigned)b, (unsigned)(b >> 32)}, make_rsrc(base, 0x7fffffffu), byte_off, 0u, 16 /* sc1 */);
}
__device__ __forceinline__ long long line16_i64(u32x4r_t v) { return (long long)(((unsigned long long)v.w << 32) | v.z); }
__device__ __forceinline__ double line16_f64(u32x4r_t v) { return __longlong_as_double((long long)(((unsigned long long)v.w << 32) | v.z)); }

// (lds_barrier(), buffer_ops.h: the workgroup barrier that orders LDS only -- the master's wave 0 has its release and its bookkeeping
// stores under way on the path from one iteration into the next)

// Release lines are shared: workgroups are dealt to the 8 XCDs round-robin, and 2^shift tiles of one XCD read the same line (shift 0: a
// line per tile).  The master's release is then 2 * 256 / 2^shift sixteen-byte stores instead of 512 -- one wave needs 1.2 us to drain 512
// of them (the last tile saw its release 1.3 us after the first store was issued, profiles/r04_C4/resident_timeline_2048_master1.txt).
__device__ __forceinline__ unsigned go_line(int tile, int shift) { return shift >= 6 ? 0u : (unsigned)((tile & 7) + 8 * ((tile >> 3) >> shift)); }   // (6: one line for all)
__device__ __forceinline__ int go_lines(int ntiles, int shift) { return shift >= 6 ? 1 : 8 * ((((ntiles - 1) >> 3) >> shift) + 1); }

// Thread 0 polls this workgroup's release line until both halves carry generation >= `gen` (bounded); the workgroup meets at a
// barrier.  Returns the leave bit (or -1: gave up) and the region means the line carries.
// (`own`: the master workgroup wrote this very release itself -- thread 0 passes what it wrote, own.gen = its generation, and no line is polled)
// Three channels: the line is 128 bytes of go_c3 and carries six pieces {generation, leave, c1_k} k = 0..2, {generation, leave, c2_k}.
template <int C> struct OwnRelease { int gen, leave; double c1[C], c2[C]; };
template <int C>
__device__ __forceinline__ int wg_wait_go(const CvhResident *rs, int bid, int gen, const CvhStepArgs &a, double *s_bc /*[1 + 2C]*/, double (&c1)[C],
                                          double (&c2)[C], const OwnRelease<C> &own);
template <>
__device__ __forceinline__ int wg_wait_go<3>(const CvhResident *rs, int bid, int gen, const CvhStepArgs &a, double *s_bc, double (&c1)[3], double (&c2)[3],
                                             const OwnRelease<3> &own)
{
  if (threadIdx.x == 0) {
    int res = -1;
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (own.gen == gen) {
      res = own.leave;
#pragma unroll
      for (int k = 0; k < 3; ++k) { m[k] = own.c1[k]; m[3 + k] = own.c2[k]; }
    } else
    for (int i = 0; i < a.res_poll_cap; ++i) {
      const unsigned line = go_line(bid, a.res_go_shift) * 128u;
      u32x4r_t g[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) g[j] = ld_line16(rs->go_c3, line + 16u * (unsigned)j);
      bool same = true;
#pragma unroll
      for (int j = 1; j < 6; ++j) same = same && g[j].x == g[0].x;
      if (same && g[0].x >= (unsigned)gen && g[0].x != 0xffffffffu) {
        res = (int)(g[0].y & 1u);
#pragma unroll
        for (int j = 0; j < 6; ++j) m[j] = line16_f64(g[j]);
        break;
      }
      if ((i & 15) == 15 && ld_agent((const unsigned *)&rs->error) != 0u) break;
      if (i >= 64) __builtin_amdgcn_s_sleep(16); else if (i >= 2) __builtin_amdgcn_s_sleep(kReleaseSleep);
    }
    if (res < 0) st_agent(const_cast<int *>(&rs->error), 1);
    s_bc[0] = (double)res;
#pragma unroll
    for (int j = 0; j < 6; ++j) s_bc[1 + j] = m[j];
  }
  lds_barrier();
  const int res = (int)s_bc[0];
#pragma unroll
  for (int k = 0; k < 3; ++k) { c1[k] = s_bc[1 + k]; c2[k] = s_bc[4 + k]; }
  lds_barrier();
  return res;
}
template <>
__device__ __forceinline__ int wg_wait_go<1>(const CvhResident *rs, int bid, int gen, const CvhStepArgs &a, double *s_bc /*[4]*/, double (&c1v)[1],
                                             double (&c2v)[1], const OwnRelease<1> &own)
{
  double &c1 = c1v[0], &c2 = c2v[0];
  if (threadIdx.x == 0) {
    int res = -1;
    double m1 = 0.0, m2 = 0.0;
    if (own.gen == gen) { res = own.leave; m1 = own.c1[0]; m2 = own.c2[0]; }
    else
    // (one poll in flight: two or four in flight sample the line more often but cost 0.5 / 0.7 us per iteration at 2048^2 -- the
    // polls of 256 workgroups compete with the arrivals and the release for the same fabric)
    for (int i = 0; i < a.res_poll_cap; ++i) {
      const unsigned line = go_line(bid, a.res_go_shift) * 64u;
      const u32x4r_t ga = ld_line16(rs->go, line), gb = ld_line16(rs->go, line + 16u);
      if (ga.x == gb.x && ga.x >= (unsigned)gen && ga.x != 0xffffffffu) { res = (int)(ga.y & 1u); m1 = line16_f64(ga); m2 = line16_f64(gb); break; }
      if ((i & 15) == 15 && ld_agent((const unsigned *)&rs->error) != 0u) break;
      if (i >= 64) __builtin_amdgcn_s_sleep(16); else if (i >= 2) __builtin_amdgcn_s_sleep(kReleaseSleep);
    }
    if (res < 0) st_agent(const_cast<int *>(&rs->error), 1);
    s_bc[0] = (double)res; s_bc[1] = m1; s_bc[2] = m2;
  }
  lds_barrier();
  const int res = (int)s_bc[0];
  c1 = s_bc[1]; c2 = s_bc[2];
  lds_barrier();
  return res;
}

// NRT: rows per wave when every tile has exactly 8 * NRT rows (2, 4, 8, 16: the march is straight-line code, row offsets are immediates, the
// band's last row is known at compile time); 0: any tile height (bands of TH / 8 rows, a loop over groups of four rows)
// One channel keeps the name it always had, csv_resident_kernel<NRT>; three channels are csv_resident_kernel<3, NRT>.  Both include the same
// body (csv_resident_body.inc): the one-channel instantiations are the instructions they were before the body knew C.
template <int NRT>
__global__ __launch_bounds__(RT_THREADS, 1) void csv_resident_kernel(const CvhStepArgs a)
{
  constexpr int C = 1;
#include "csv_resident_body.inc"
}
template <int C, int NRT>
__global__ __launch_bounds__(RT_THREADS, 1) void csv_resident_kernel(const CvhStepArgs a)
{
#include "csv_resident_body.inc"
}

}  // namespace

size_t cvh_resident_lds_bytes(int channels) { return channels == 3 ? ResSmem<3>::bytes : ResSmem<1>::bytes; }
int cvh_resident_tile_w() { return RT_W; }
int cvh_resident_tile_hmax(int channels) { return rt_hmax(channels == 3 ? 3 : 1); }
int cvh_resident_halo_doubles() { return RT_HALO; }

namespace {
typedef void (*ResKernel)(const CvhStepArgs);
ResKernel res_kernel(int channels, int band_rows)
{
  if (channels == 3) {
    switch (band_rows) {           // (8 x 16 rows is more than a three-channel tile may have)
      case 0: return csv_resident_kernel<3, 0>;
      case 2: return csv_resident_kernel<3, 2>;
      case 4: return csv_resident_kernel<3, 4>;
      case 8: return csv_resident_kernel<3, 8>;
    }
    return nullptr;
  }
  switch (band_rows) {
    case 0: return csv_resident_kernel<0>;
    case 2: return csv_resident_kernel<2>;
    case 4: return csv_resident_kernel<4>;
    case 8: return csv_resident_kernel<8>;
    case 16: return csv_resident_kernel<16>;
  }
  return nullptr;
}
}  // namespace

// Workgroups of the resident kernel one CU holds (0: not launchable, e.g. the LDS request was refused): the least over the flavours.
int cvh_resident_blocks_per_cu(int channels)
{
  static int cached_c[2] = {-1, -1};
  int &cached = cached_c[channels == 3 ? 1 : 0];
  if (cached >= 0) return cached;
  const size_t lds = cvh_resident_lds_bytes(channels);
  int least = 1 << 30;
  for (int nr = 0; nr <= 16; nr = nr ? 2 * nr : 2) {
    const void *k = reinterpret_cast<const void *>(res_kernel(channels, nr));
    if (!k) continue;
    int n = 0;
    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, RT_THREADS, lds) != hipSuccess) {
      (void)hipGetLastError();
      return cached = 0;
    }
    if (n < least) least = n;
  }
  return cached = least;
}

// `channels` selects the instantiation (the arguments themselves do not carry the count)
hipError_t cvh_launch_resident(const CvhStepArgs &a, int channels, hipStream_t s)
{
  const ResKernel kern = res_kernel(channels, a.res_band_rows);
  if (!kern) return hipErrorInvalidValue;
  const size_t lds = cvh_resident_lds_bytes(channels);
  if (a.note) {
    if (channels == 3) cvh_fill_note(a.note, (unsigned)(a.tiles_x * a.tiles_y), RT_THREADS, lds, "csv_resident_kernel<3, %d>", a.res_band_rows);
    else cvh_fill_note(a.note, (unsigned)(a.tiles_x * a.tiles_y), RT_THREADS, lds, "csv_resident_kernel<%d>", a.res_band_rows);
    return hipSuccess;
  }
  CvhStepArgs copy = a;
  void *params[] = {&copy};
  return hipLaunchCooperativeKernel(reinterpret_cast<const void *>(kern), dim3(a.tiles_x * a.tiles_y), dim3(RT_THREADS), params, (unsigned)lds, s);
}
