// init_kernels.hip — device-side initial level sets (gfx950): the histogram of the grey values g(p) = sum_k I_k(p) of a context's planes,
// and the threshold / rectangle / disk starts (include/chanvese_hip.h, "Device-side initial level sets").  Batch kernels over io_run.hip's
// member table like the ones in io_kernels.hip: ONE grid serves N members of any mix of shapes and channel counts, a member owning the
// workgroups first .. first + nblk - 1; the single-context entry points launch the same kernels with a table of one member.
#include "cvh_internal.h"

namespace {

// everything the table points at is global memory (the contexts' own buffers): global_load / global_store, not flat operations
#define CVH_GLOBAL __attribute__((address_space(1)))
typedef CVH_GLOBAL const uint8_t *gbytes_in;
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

// the member whose section holds this workgroup (first is ascending, tab[0].first == 0): wave-uniform
__device__ __forceinline__ int init_member(const CvhIoMember *tab, int nmem)
{
  int lo = 0, hi = nmem - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One grey value per live lane is counted in the workgroup's LDS histogram.  A flat image (or a flat region: a sky, a mask border) sends
// all 64 lanes of the instruction to ONE counter, and same-address LDS atomics serialise.  So equal values are aggregated within the
// wave first: the first live lane's value is broadcast, the lanes that hold it are counted with a ballot, and that lane alone adds the
// count.  A round is worth its two ballots only while it retires a good share of the wave, so it repeats (at most four times: up to
// four dominant values) while the leader's value covers at least a quarter of the lanes still live; the others add 1 each.  Every
// condition is wave-uniform.  Called by all 64 lanes of a wave together (live = false for a lane without a pixel).
__device__ __forceinline__ void count_grey(unsigned *sh, unsigned v, bool live, int lane)
{
  for (int round = 0; round < 4; ++round) {
    const unsigned long long todo = __ballot(live);
    if (!todo) return;
    const int lead = __ffsll((long long)todo) - 1;
    const unsigned lv = (unsigned)__shfl((int)v, lead, 64);
    const bool same = live && v == lv;
    const int c = __popcll(__ballot(same));
    if (4 * c < __popcll(todo)) break;
    if (lane == lead) atomicAdd(&sh[lv], (unsigned)c);
    live = live && !same;
  }
  if (live) atomicAdd(&sh[v], 1u);
}

__device__ __forceinline__ void add_piece(unsigned g[16], const v4u p)
{
  const unsigned wds[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int b = 0; b < 4; ++b) g[4 * i + b] += (wds[i] >> (8 * b)) & 0xffu;
  }
}

// hist[v] = number of pixels with g = v, v = 0 .. 255 C, into the member's 32-bit counters (m->sums, zeroed by the host before the
// launch).  A lane reads one 16-byte piece of every plane per trip -- all C planes of a pixel in the same lane -- and counts in LDS; the
// workgroup flushes its non-empty bins once with 32-bit global atomics (integer adds: the result does not depend on the order).  The
// n % 16 last pixels go pixel by pixel in the first wave of the member's first workgroup.  A workgroup counts fewer than 2^32 pixels
// (the host refuses h * w >= 2^32), so no counter wraps.
__global__ void __launch_bounds__(CVH_BLOCK) init_histogram_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned sh[CVH_HIST_MAX_BINS];
  const CvhIoMember *m = tab + init_member(tab, nmem);
  const int C = m->C, B = 255 * C + 1;
  for (int b = (int)threadIdx.x; b < B; b += CVH_BLOCK) sh[b] = 0;
  __syncthreads();
  const size_t n = m->n, pieces = n / 16, stride = (size_t)m->nblk * CVH_BLOCK;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wg = (int)(blockIdx.x - m->first);
  const gbytes_in plane[3] = {(gbytes_in)m->plane[0], (gbytes_in)m->plane[1], (gbytes_in)m->plane[2]};
  // the 64 lanes of a wave make the same trips (a lane past the last piece rides along idle): count_grey's ballots see whole waves
  for (size_t base = (size_t)wg * CVH_BLOCK + 64 * (size_t)wave; base < pieces; base += stride) {
    const size_t q = base + lane;
    const bool live = q < pieces;
    unsigned g[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (live)
      for (int k = 0; k < C; ++k) add_piece(g, ((CVH_GLOBAL const v4u *)plane[k])[q]);
#pragma unroll
    for (int i = 0; i < 16; ++i) count_grey(sh, g[i], live, lane);
  }
  if (wg == 0 && wave == 0) {
    const size_t q = pieces * 16 + lane;
    const bool live = q < n;
    unsigned g = 0;
    if (live)
      for (int k = 0; k < C; ++k) g += plane[k][q];
    count_grey(sh, g, live, lane);
  }
  __syncthreads();
  unsigned *hist = (unsigned *)m->sums;
  for (int b = (int)threadIdx.x; b < B; b += CVH_BLOCK) {
    const unsigned c = sh[b];
    if (c) atomicAdd(&hist[b], c);
  }
}

// is pixel (row, col), whose grey value is g, inside?  (mode is wave-uniform: a member's)
__device__ __forceinline__ bool start_inside(const CvhInitStart &p, unsigned row, unsigned col, unsigned g)
{
  if (p.mode == CVH_START_THRESHOLD) return (long long)g > p.a;
  if (p.mode == CVH_START_RECT) return (long long)col >= p.a && (long long)col < p.b && (long long)row >= p.c && (long long)row < p.d;
  const long long dx = (long long)col - p.a, dy = (long long)row - p.b, r = p.c;   // r < 2^31
  if (dx > r || dx < -r || dy > r || dy < -r) return false;   // (and so the sum of the squares below stays under 2^63)
  return dx * dx + dy * dy <= r * r;
}

// The threshold / rectangle / disk start of N members: u(p) = inside or outside (any doubles, selected bit for bit), two pixels per
// lane and trip, written with one 16-byte store; an odd last pixel goes alone.  par[i] is member i's start (cvh_internal.h).  The
// threshold mode reads the two pixels' bytes of every plane (one 2-byte load per plane).  A member's first workgroup also clears what a
// new run clears (reset_run_impl), exactly as io_checkerboard_kernel: the four run words of its state block and the chain-mode sum set
// behind the current one.
__global__ void __launch_bounds__(CVH_BLOCK) init_start_kernel(const CvhIoMember *tab, const CvhInitStart *par, int nmem)
{
  const int mi = init_member(tab, nmem);
  const CvhIoMember *m = tab + mi;
  const CvhInitStart p = par[mi];
  const int wg = (int)(blockIdx.x - m->first), C = m->C;
  if (wg == 0) {
    if (threadIdx.x < 4) ((CVH_GLOBAL int *)m->state_zero)[threadIdx.x] = 0;
    if (threadIdx.x < 64) ((CVH_GLOBAL long long *)m->chain_zero)[threadIdx.x] = 0;
  }
  const size_t n = m->n, pairs = n / 2;   // n < 2^32 (the host refuses larger planes): pixel indices are 32-bit
  const unsigned w = (unsigned)m->w;
  const size_t t0 = (size_t)wg * CVH_BLOCK + threadIdx.x, stride = (size_t)m->nblk * CVH_BLOCK;
  const gbytes_in plane[3] = {(gbytes_in)m->plane[0], (gbytes_in)m->plane[1], (gbytes_in)m->plane[2]};
  CVH_GLOBAL double *u = (CVH_GLOBAL double *)m->dst;
  const bool grey = p.mode == CVH_START_THRESHOLD;
  for (size_t q = t0; q < pairs; q += stride) {
    const unsigned idx = (unsigned)(2 * q);
    unsigned row = idx / w, col = idx - row * w;
    unsigned g0 = 0, g1 = 0;
    if (grey)
      for (int k = 0; k < C; ++k) {
        const unsigned two = *(CVH_GLOBAL const unsigned short *)(plane[k] + idx);   // (idx is even, the planes are 256-byte aligned)
        g0 += two & 0xffu; g1 += two >> 8;
      }
    const bool in0 = start_inside(p, row, col, g0);
    if (++col == w) { col = 0; ++row; }
    const bool in1 = start_inside(p, row, col, g1);
    const v2d o = {in0 ? p.inside : p.outside, in1 ? p.inside : p.outside};
    ((CVH_GLOBAL v2d *)u)[q] = o;
  }
  if ((n & 1) && t0 == 0) {
    const unsigned idx = (unsigned)(n - 1), row = idx / w, col = idx - row * w;
    unsigned g = 0;
    if (grey)
      for (int k = 0; k < C; ++k) g += plane[k][idx];
    u[idx] = start_inside(p, row, col, g) ? p.inside : p.outside;
  }
}

}  // namespace

// workgroups of a member of n pixels in the start kernel (two pixels per lane and trip)
unsigned cvh_init_start_blocks(size_t n)
{
  const size_t b = (n / 2 + CVH_BLOCK) / CVH_BLOCK;
  return (unsigned)(b > 2048 ? 2048 : b);
}

hipError_t cvh_launch_init_histogram(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(init_histogram_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}

hipError_t cvh_launch_init_start(const CvhIoMember *tab, const CvhInitStart *par, int nmem, unsigned grid, hipStream_t s)
{
  hipLaunchKernelGGL(init_start_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, par, nmem);
  return hipGetLastError();
}
