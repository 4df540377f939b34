// smooth_kernels.hip — the weighted window on the device (gfx950): plane k of a member is COPY, BLUR or DETAIL of a plane of its source
// context under a symmetric separable kernel of 2 R + 1 taps, indices clamped to the plane (include/chanvese_hip.h, "Smoothing": exact
// integers, the two roundings in smooth_math.h).  Batch kernels over io_run.hip's member table like local_kernels.hip's: ONE grid serves
// N members of any mix of shapes, channel counts, radii, taps and codes, a member owning the workgroups first .. first + nblk - 1; both
// launches read the same table, and a member's taps (CVH_SMOOTH_RADIUS_MAX + 1 entries of 16 bits, zero behind R) sit behind src2.
// The staging of a row span and the decoder of a row item are window_device.h's.  A weighted window has no running sum, so the work
// per pixel grows with R: R + 1 multiplications per pass, the taps paired as t[i] (x[-i] + x[+i]).
//   row pass     per source plane that a BLUR or DETAIL plane reads.  A workgroup stages a row segment's span, expands it into bytes with
//                the clamp applied (ext[i] is column clamp(c0 - R + i)), and a lane adds up four columns 256 apart; v = (a + 64) >> 7
//                goes as 16 bits into the member's workspace, rows cvh_window_pitch(w) entries apart.
//   column pass  a workgroup takes a band of 256 - 2 R rows x kSmoothStrip columns per trip and holds the band's rows of v and R rows
//                on either side, clamped, in LDS: kSmoothTile x 64 x 2 bytes = 32 KiB.  A lane owns a column; a wave takes four rows at a
//                time, so that a tap is fetched once for four sums.  It writes the member's planes, the COPY planes included.
// The taps are wave-uniform: lane i of every wave holds t[i] and a sum reads it with v_readlane, into a scalar register.
// The source is only read.  No kernel waits for another workgroup; the column launch follows the row launch on the same stream.
#include "window_device.h"
#include "smooth_math.h"

namespace {

constexpr int kSmoothStrip = CVH_SMOOTH_STRIP, kSmoothTile = CVH_SMOOTH_TILE_ROWS;
constexpr int kExt = kSegment + 2 * CVH_SMOOTH_RADIUS_MAX;   // bytes of a segment's clamped span
static_assert(kSmoothStrip == 64, "a lane of the column pass owns one column");
static_assert(CVH_SMOOTH_RADIUS_MAX + 1 <= 64, "lane i of a wave holds tap i");
static_assert(CVH_SMOOTH_RADIUS_MAX <= CVH_LOCAL_RADIUS_MAX, "window_device.h's span holds a segment's");
static_assert(kSmoothTile - 2 * CVH_SMOOTH_RADIUS_MAX >= 4, "a band has rows at every radius");
static_assert(kSegment == 4 * CVH_BLOCK, "a lane of the row pass takes four columns of a segment");
static_assert(kSmoothTile * 255ll * 255 < (1ll << 32), "a lane's 32-bit plane sums hold one trip");

typedef CVH_GLOBAL const uint16_t *ghalves_in;
typedef CVH_GLOBAL uint16_t *ghalves_out;

__device__ __forceinline__ int what_of(const CvhIoMember *m, int k) { return (m->interleaved >> (2 * k)) & 3; }

// bit s: a BLUR or DETAIL plane of the member reads plane s of the source
__device__ __forceinline__ unsigned planes_read(const CvhIoMember *m)
{
  unsigned need = 0;
  for (int k = 0; k < m->C; ++k)
    if (what_of(m, k) != CVH_SMOOTH_COPY) need |= 1u << source_of(m, k);
  return need;
}

// lane i holds t[i] (0 behind R); tap(mine, i) with a wave-uniform i is a scalar
__device__ __forceinline__ unsigned my_tap(const CvhIoMember *m, int R)
{
  const int lane = threadIdx.x & 63;
  return lane <= R ? (unsigned)((ghalves_in)m->src2)[lane] : 0u;
}
__device__ __forceinline__ unsigned tap(unsigned mine, int i) { return (unsigned)__builtin_amdgcn_readlane((int)mine, i); }

__global__ void __launch_bounds__(CVH_BLOCK) smooth_rows_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned raw[kRawWords];
  __shared__ uint8_t ext[kExt];
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const unsigned need = planes_read(m);
  if (!need) return;   // (the whole workgroup)
  const int h = m->h, w = m->w, R = m->h2;
  const int nseg = (w + kSegment - 1) / kSegment;
  const size_t pitch = cvh_window_pitch(w), slot = cvh_smooth_slot_bytes(h, w);
  const unsigned long long per_plane = (unsigned long long)h * nseg, items = per_plane * __popc(need);
  const int tid = threadIdx.x;
  const unsigned taps = my_tap(m, R), t0 = tap(taps, 0);
  for (unsigned long long item = blockIdx.x - m->first; item < items; item += m->nblk) {
    const RowItem it = row_item(item, per_plane, nseg);
    const int r = it.r, s = nth_set_bit<CVH_MAX_CHANNELS>(need, it.nth);   // the nth plane that is read
    const gbytes_in plane = (gbytes_in)m->src + (size_t)s * m->src_stride;
    const int c0 = it.g * kSegment, cend = min(c0 + kSegment, w), len = cend - c0;
    const RowSpan sp = stage_row_span(raw, plane, r, (size_t)w, c0, cend, R, w, 0u);
    for (int i = tid; i < len + 2 * R; i += CVH_BLOCK)   // first <= the clamped column <= last
      ext[i] = (uint8_t)span_byte(raw, sp, min(max(c0 - R + i, 0), w - 1) - sp.first);
    __syncthreads();
    int x[4];
    unsigned a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { x[j] = min(tid + CVH_BLOCK * j, len - 1) + R; a[j] = t0 * ext[x[j]]; }
    for (int i = 1; i <= R; ++i) {
      const unsigned t = tap(taps, i);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] += t * ((unsigned)ext[x[j] - i] + (unsigned)ext[x[j] + i]);
    }
    const ghalves_out q = (ghalves_out)((CVH_GLOBAL uint8_t *)m->dst + (size_t)s * slot) + (size_t)r * pitch + c0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (tid + CVH_BLOCK * j < len) q[tid + CVH_BLOCK * j] = (uint16_t)cvh_smooth_row(a[j]);
    __syncthreads();   // the next trip rewrites the staging
  }
}

__global__ void __launch_bounds__(CVH_BLOCK) smooth_columns_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ uint16_t tile[kSmoothTile * kSmoothStrip];
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const int h = m->h, w = m->w, R = m->h2, C = m->C, Cs = m->w2;
  const int band = cvh_smooth_band_rows(R);
  const int nstrip = (w + kSmoothStrip - 1) / kSmoothStrip, nband = (h + band - 1) / band;
  const size_t pitch = cvh_window_pitch(w), slot = cvh_smooth_slot_bytes(h, w);
  const unsigned long long items = (unsigned long long)nband * nstrip;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned taps = my_tap(m, R), t0 = tap(taps, 0);
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  for (unsigned long long item = blockIdx.x - m->first; item < items; item += m->nblk) {
    const int r0 = (int)(item / nstrip) * band, r1 = min(r0 + band, h), rows = r1 - r0;
    const int c = (int)(item % nstrip) * kSmoothStrip + lane;
    const bool inside = c < w;
    const size_t cl = (size_t)min(c, w - 1);
    unsigned s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
    for (int s = 0; s < Cs; ++s) {
      unsigned mine = 0, blur_of = 0, detail_of = 0;   // the member's planes that come from source plane s, by code (uniform)
#pragma unroll
      for (int k = 0; k < CVH_MAX_CHANNELS; ++k)
        if (k < C && source_of(m, k) == s) {
          mine |= 1u << k;
          if (what_of(m, k) == CVH_SMOOTH_BLUR) blur_of |= 1u << k;
          if (what_of(m, k) == CVH_SMOOTH_DETAIL) detail_of |= 1u << k;
        }
      if (!mine) continue;
      const bool smooth = (blur_of | detail_of) != 0, bytes = (mine & ~blur_of) != 0;
      const gbytes_in plane = (gbytes_in)m->src + (size_t)s * m->src_stride;
      if (smooth) {   // tile row j is row clamp(r0 - R + j) of v, j < rows + 2 R <= kSmoothTile
        const ghalves_in v = (ghalves_in)((CVH_GLOBAL const uint8_t *)m->dst + (size_t)s * slot);
        __syncthreads();   // the trip before has read the tile
        for (int j = wave; j < rows + 2 * R; j += CVH_BLOCK / 64)
          tile[j * kSmoothStrip + lane] = v[(size_t)min(max(r0 - R + j, 0), h - 1) * pitch + cl];
        __syncthreads();
      }
      for (int y0 = 4 * wave; y0 < rows; y0 += 4 * (CVH_BLOCK / 64)) {
        int at[4];   // the tile entry of the lane's column in the four rows' own row (a row behind the band repeats its last)
        unsigned b[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) at[j] = (min(y0 + j, rows - 1) + R) * kSmoothStrip + lane;
        if (smooth) {
#pragma unroll
          for (int j = 0; j < 4; ++j) b[j] = t0 * tile[at[j]];
          for (int i = 1; i <= R; ++i) {
            const unsigned t = tap(taps, i);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] += t * ((unsigned)tile[at[j] - i * kSmoothStrip] + (unsigned)tile[at[j] + i * kSmoothStrip]);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (y0 + j >= rows || !inside) continue;
          const size_t px = (size_t)(r0 + y0 + j) * w + (size_t)c;
          const unsigned p = bytes ? plane[px] : 0u, blur = cvh_smooth_blur(b[j]), detail = cvh_smooth_detail(p, blur);
#pragma unroll
          for (int k = 0; k < CVH_MAX_CHANNELS; ++k)
            if ((mine >> k) & 1u) {
              const unsigned o = ((blur_of >> k) & 1u) ? blur : ((detail_of >> k) & 1u) ? detail : p;
              ((gbytes_out)m->plane[k])[px] = (uint8_t)o;
              s1[k] += o; s2[k] += o * o;
            }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) flush(acc + 2 * k, s1[k], s2[k]);
  }
  add_sums(acc, C, m->sums);
}

}  // namespace

// workgroups of a member: the larger of what the two passes share out, a trip per workgroup in both; the rest is taken on further trips
unsigned cvh_smooth_blocks(int h, int w, int R, int planes_read)
{
  const size_t band = (size_t)cvh_smooth_band_rows(R);
  const size_t rows = (size_t)planes_read * (size_t)h * (((size_t)w + kSegment - 1) / kSegment);
  const size_t cols = (((size_t)h + band - 1) / band) * (((size_t)w + kSmoothStrip - 1) / kSmoothStrip);
  const size_t b = rows > cols ? rows : cols;
  return (unsigned)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

hipError_t cvh_launch_smooth(const CvhIoMember *tab, int nmem, unsigned grid, unsigned passes, hipStream_t s)
{
  if (passes) hipLaunchKernelGGL(smooth_rows_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  hipLaunchKernelGGL(smooth_columns_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}
