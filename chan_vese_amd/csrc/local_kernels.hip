// local_kernels.hip — local mean and local deviation planes on the device (gfx950): plane k of a member is COPY, MEAN or DEV of a plane
// of its source context over the (2 R + 1)^2 window truncated at the border (include/chanvese_hip.h, "Local statistics": exact integers,
// local_math.h).  Batch kernels over io_run.hip's member table like colour_kernels.hip's: ONE grid serves N members of any mix of shapes,
// channel counts, radii and codes, a member owning the workgroups first .. first + nblk - 1; both launches read the same table.  The
// passes' geometry, the staging of a row span and the sharing out of items are window_device.h's; here are the arithmetic and the writer.
// The window sums are separable, so the work per pixel does not grow with R^2:
//   row pass     per source plane that a MEAN or DEV plane reads, the horizontal window sums of p (16-bit) and p^2 (32-bit) go into the
//                member's workspace.  Of the staged span a lane adds up kRowLane consecutive bytes, a wave scan and a carry across the
//                four waves turn that into the inclusive prefix sums of the span in LDS, and a pixel's window sum is the difference
//                of two prefix entries.
//   column pass  a band is kBand rows.  The lane holds the vertical sums of its columns' row sums in registers (both fit 32 bits:
//                255^2 * 255^2 < 2^32), fills them from the 2 R + 1 rows about the band's first row and marches down, adding row
//                r + R + 1 and subtracting row r - R, both clipped; a row of the workspace is read as one 16-byte and one 8-byte piece
//                per lane.  It writes the member's planes, the COPY planes included.
// The source is only read.  No kernel waits for another workgroup; the column launch follows the row launch on the same stream.
#include "window_device.h"
#include "local_math.h"

namespace {

typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef CVH_GLOBAL const uint16_t *ghalves_in;

__device__ __forceinline__ int what_of(const CvhIoMember *m, int k) { return (m->interleaved >> (2 * k)) & 3; }

// bit s: a MEAN or DEV plane of the member reads plane s of the source
__device__ __forceinline__ unsigned planes_read(const CvhIoMember *m)
{
  unsigned need = 0;
  for (int k = 0; k < m->C; ++k)
    if (what_of(m, k) != CVH_LOCAL_COPY) need |= 1u << source_of(m, k);
  return need;
}

__global__ void __launch_bounds__(CVH_BLOCK) local_rows_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned raw[kRawWords];
  __shared__ unsigned pre1[kRowLane * CVH_BLOCK], pre2[kRowLane * CVH_BLOCK];
  __shared__ unsigned wave_total[CVH_BLOCK / 64][2];
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const unsigned need = planes_read(m);
  if (!need) return;   // (the whole workgroup)
  const int h = m->h, w = m->w, R = m->h2;
  const int nseg = (w + kSegment - 1) / kSegment;
  const size_t pitch = cvh_window_pitch(w), slot = cvh_local_slot_bytes(h, w);
  const unsigned long long per_plane = (unsigned long long)h * nseg, items = per_plane * __popc(need);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (unsigned long long item = blockIdx.x - m->first; item < items; item += m->nblk) {
    const RowItem it = row_item(item, per_plane, nseg);
    const int r = it.r, s = nth_set_bit<CVH_MAX_CHANNELS>(need, it.nth);   // the nth plane that is read
    const gbytes_in plane = (gbytes_in)m->src + (size_t)s * m->src_stride;
    const int c0 = it.g * kSegment, cend = min(c0 + kSegment, w);
    const RowSpan sp = stage_row_span(raw, plane, r, (size_t)w, c0, cend, R, w, 0u);
    unsigned p1[kRowLane], p2[kRowLane], t1 = 0, t2 = 0;
#pragma unroll
    for (int j = 0; j < kRowLane; ++j) {
      const int i = kRowLane * tid + j;
      const unsigned x = i < sp.len ? span_byte(raw, sp, i) : 0u;
      t1 += x; t2 += x * x;
      p1[j] = t1; p2[j] = t2;
    }
    unsigned i1 = t1, i2 = t2;   // inclusive scan of the lanes' totals over the wave
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned a = __shfl_up(i1, off, 64), b = __shfl_up(i2, off, 64);
      if (lane >= off) { i1 += a; i2 += b; }
    }
    if (lane == 63) { wave_total[wave][0] = i1; wave_total[wave][1] = i2; }
    __syncthreads();
    unsigned base1 = i1 - t1, base2 = i2 - t2;   // what lies in front of this lane's bytes
    for (int v = 0; v < wave; ++v) { base1 += wave_total[v][0]; base2 += wave_total[v][1]; }
#pragma unroll
    for (int j = 0; j < kRowLane; ++j) { pre1[kRowLane * tid + j] = base1 + p1[j]; pre2[kRowLane * tid + j] = base2 + p2[j]; }
    __syncthreads();
    CVH_GLOBAL unsigned *const q2 = (CVH_GLOBAL unsigned *)((CVH_GLOBAL uint8_t *)m->dst + (size_t)s * slot);
    CVH_GLOBAL uint16_t *const q1 = (CVH_GLOBAL uint16_t *)(q2 + (size_t)h * pitch);
    for (int c = c0 + tid; c < cend; c += CVH_BLOCK) {
      const int lo = max(c - R, 0), hi = min(c + R, w - 1);   // first <= lo <= hi <= last
      const unsigned b1 = lo > sp.first ? pre1[lo - 1 - sp.first] : 0u, b2 = lo > sp.first ? pre2[lo - 1 - sp.first] : 0u;
      const size_t at = (size_t)r * pitch + c;
      q2[at] = pre2[hi - sp.first] - b2;
      q1[at] = (uint16_t)(pre1[hi - sp.first] - b1);
    }
    __syncthreads();   // the next trip rewrites the staging
  }
}

struct RowSums { unsigned s1[4], s2[4]; };

// the row sums of a lane's four columns in row r of a slot
__device__ __forceinline__ RowSums load_row(gwords_in q2, ghalves_in q1, size_t at)
{
  const v4u a = *(CVH_GLOBAL const v4u *)(q2 + at);
  const v2u b = *(CVH_GLOBAL const v2u *)(q1 + at);
  return RowSums{{b.x & 0xffffu, b.x >> 16, b.y & 0xffffu, b.y >> 16}, {a.x, a.y, a.z, a.w}};
}

__global__ void __launch_bounds__(CVH_BLOCK) local_columns_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const int h = m->h, w = m->w, R = m->h2, C = m->C, Cs = m->w2;
  const int nstrip = (w + kStrip - 1) / kStrip, nband = (h + kBand - 1) / kBand;
  const size_t pitch = cvh_window_pitch(w), slot = cvh_local_slot_bytes(h, w);
  const unsigned long long items = (unsigned long long)nband * nstrip;
  const unsigned long long nwaves = wave_item_step(m, CVH_BLOCK / 64);
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  for (unsigned long long item = first_wave_item(m, CVH_BLOCK / 64); item < items; item += nwaves) {
    const ColumnItem it = column_item(item, nstrip, kBand, h, w);
    const int r0 = it.r0, r1 = it.r1, cc = it.cc, valid = it.valid;
    unsigned nc[4];   // columns of a pixel's window
#pragma unroll
    for (int j = 0; j < 4; ++j) nc[j] = (unsigned)(min(cc + j + R, w - 1) - max(cc + j - R, 0) + 1);
    unsigned s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
    for (int s = 0; s < Cs; ++s) {
      unsigned mine = 0, mean_of = 0, dev_of = 0;   // the member's planes that come from source plane s, by code (wave-uniform)
#pragma unroll
      for (int k = 0; k < CVH_MAX_CHANNELS; ++k)
        if (k < C && source_of(m, k) == s) {
          mine |= 1u << k;
          if (what_of(m, k) == CVH_LOCAL_MEAN) mean_of |= 1u << k;
          if (what_of(m, k) == CVH_LOCAL_DEV) dev_of |= 1u << k;
        }
      if (!mine || valid <= 0) continue;
      const bool stats = (mean_of | dev_of) != 0, copies = (mine & ~(mean_of | dev_of)) != 0;
      const gbytes_in plane = (gbytes_in)m->src + (size_t)s * m->src_stride;
      const gwords_in q2 = (gwords_in)((CVH_GLOBAL const uint8_t *)m->dst + (size_t)s * slot);
      const ghalves_in q1 = (ghalves_in)(q2 + (size_t)h * pitch);
      unsigned v1[4] = {0, 0, 0, 0}, v2[4] = {0, 0, 0, 0};   // sums over the window's rows of the row sums
      if (stats)
        for (int rr = max(r0 - R, 0); rr <= min(r0 + R, h - 1); ++rr) {
          const RowSums a = load_row(q2, q1, (size_t)rr * pitch + cc);
#pragma unroll
          for (int j = 0; j < 4; ++j) { v1[j] += a.s1[j]; v2[j] += a.s2[j]; }
        }
      for (int r = r0; r < r1; ++r) {
        const size_t at = (size_t)r * w + cc;
        unsigned copy = 0, mean = 0, dev = 0;
        if (copies) copy = load_bytes(plane + at, valid);
        if (stats) {
          const unsigned nr = (unsigned)(min(r + R, h - 1) - max(r - R, 0) + 1);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < valid) {
              const unsigned n = nr * nc[j];
              if (mean_of) mean |= cvh_local_mean(n, v1[j]) << (8 * j);
              if (dev_of) dev |= cvh_local_dev(n, v1[j], v2[j]) << (8 * j);
            }
          if (r + R + 1 <= h - 1) {
            const RowSums a = load_row(q2, q1, (size_t)(r + R + 1) * pitch + cc);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v1[j] += a.s1[j]; v2[j] += a.s2[j]; }
          }
          if (r - R >= 0) {
            const RowSums a = load_row(q2, q1, (size_t)(r - R) * pitch + cc);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v1[j] -= a.s1[j]; v2[j] -= a.s2[j]; }
          }
        }
#pragma unroll
        for (int k = 0; k < CVH_MAX_CHANNELS; ++k)
          if ((mine >> k) & 1u) {
            const unsigned v = ((mean_of >> k) & 1u) ? mean : ((dev_of >> k) & 1u) ? dev : copy;
            store_bytes((gbytes_out)m->plane[k] + at, v, valid);
#pragma unroll
            for (int j = 0; j < 4; ++j) { const unsigned x = (v >> (8 * j)) & 0xffu; s1[k] += x; s2[k] += x * x; }
          }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) flush(acc + 2 * k, s1[k], s2[k]);
  }
  add_sums(acc, C, m->sums);
}

}  // namespace

// workgroups of a member: the larger of what the two passes share out, a trip per workgroup (rows) or per wave (columns); the rest is
// taken on further trips
unsigned cvh_local_blocks(int h, int w, int planes_read)
{
  const size_t rows = (size_t)planes_read * (size_t)h * (((size_t)w + kSegment - 1) / kSegment);
  const size_t cols = (((size_t)h + kBand - 1) / kBand) * (((size_t)w + kStrip - 1) / kStrip);
  const size_t by_rows = rows, by_cols = (cols + CVH_BLOCK / 64 - 1) / (CVH_BLOCK / 64), b = by_rows > by_cols ? by_rows : by_cols;
  return (unsigned)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

hipError_t cvh_launch_local(const CvhIoMember *tab, int nmem, unsigned grid, unsigned passes, hipStream_t s)
{
  if (passes) hipLaunchKernelGGL(local_rows_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  hipLaunchKernelGGL(local_columns_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}
