// window_device.h — what the kernels of the windowed-plane calls share (local_kernels.hip, rank_kernels.hip; host side window_run.hip):
// plane k of a member comes from plane min(k, C_src - 1) of its source over the (2 R + 1)^2 window truncated at the border, by row and
// column passes over ONE member table.  In a row pass a workgroup takes a row segment of kSegment columns per trip, whose bytes and R
// columns on either side (the span) are staged in LDS by aligned words; in a column pass a wave takes a band of rows x kStrip columns
// per trip, a lane four adjacent columns.  Here: that geometry, bytes and words at any address, the nth set bit of a job mask, the
// staging of a span and the decoders of a pass's items.  The arithmetic and the writing of the member's planes with their sums (a
// lane's 32-bit sums of a trip, flush, add_sums: io_device.h) are in a family's own file.
#pragma once
#include "io_device.h"

namespace {

constexpr int kSegment = CVH_WINDOW_SEGMENT, kBand = CVH_WINDOW_BAND, kStrip = CVH_WINDOW_STRIP;
constexpr int kSpan = kSegment + 2 * CVH_LOCAL_RADIUS_MAX;        // bytes a segment's windows read at most
constexpr int kRowLane = (kSpan + CVH_BLOCK - 1) / CVH_BLOCK;     // consecutive bytes of the span a lane of the row pass takes
constexpr int kRawWords = (kSpan + 3) / 4 + 1;                    // the span as aligned words: up to 3 bytes in front of it
static_assert(CVH_RANK_RADIUS_MAX == CVH_LOCAL_RADIUS_MAX, "one span serves both families");
static_assert(kStrip == 4 * 64, "a lane of the column pass owns four columns");

typedef unsigned u32_any __attribute__((aligned(1)));
typedef CVH_GLOBAL const unsigned *gwords_in;
typedef CVH_GLOBAL unsigned *gwords_out;

// the source plane that plane k of the member comes from
__device__ __forceinline__ int source_of(const CvhIoMember *m, int k) { return min(k, m->w2 - 1); }

// the nth set bit of a mask of kBits bits (CVH_MAX_CHANNELS source planes, or twice as many jobs), nth < its population count: wave-uniform
template <int kBits>
__device__ __forceinline__ int nth_set_bit(unsigned mask, int nth)
{
  int at = 0;
  for (int b = 0, seen = 0; b < kBits; ++b)
    if ((mask >> b) & 1u) { if (seen == nth) at = b; ++seen; }
  return at;
}

// `valid` bytes (1 .. 4) of a plane at any byte address, as a word whose other bytes are zero
__device__ __forceinline__ unsigned load_bytes(gbytes_in p, int valid)
{
  if (valid == 4) return *(CVH_GLOBAL const u32_any *)p;
  unsigned v = 0;
  for (int j = 0; j < valid; ++j) v |= (unsigned)p[j] << (8 * j);
  return v;
}
__device__ __forceinline__ void store_bytes(gbytes_out p, unsigned v, int valid)
{
  if (valid == 4) { *(CVH_GLOBAL u32_any *)p = v; return; }
  for (int j = 0; j < valid; ++j) p[j] = (uint8_t)(v >> (8 * j));
}

// The span of a row segment: columns first .. last of row r are what the windows of columns c0 .. cend - 1 read; byte i of the span sits
// `mis` bytes into the staged words.  stage_row_span stages it (rows `stride` bytes apart) in raw[kRawWords] by aligned words, every word
// XORed with `flip`, and waits for the workgroup.  The last word ends at or before the row's end rounded up to 4: inside the plane's
// own padding (cvh_create pads every plane to a multiple of 256 bytes) or inside a workspace row's pitch.
struct RowSpan { int first, last, len, mis; };
__device__ __forceinline__ RowSpan stage_row_span(unsigned *raw, gbytes_in plane, int r, size_t stride, int c0, int cend, int R, int w, unsigned flip)
{
  const int first = max(c0 - R, 0), last = min(cend - 1 + R, w - 1), len = last - first + 1;
  const size_t a0 = (size_t)r * stride + first, al = a0 & ~(size_t)3;
  const int mis = (int)(a0 - al), nwords = (mis + len + 3) / 4;
  for (int t = threadIdx.x; t < nwords; t += CVH_BLOCK) raw[t] = *(gwords_in)(plane + al + 4 * (size_t)t) ^ flip;
  __syncthreads();
  return RowSpan{first, last, len, mis};
}
__device__ __forceinline__ unsigned span_byte(const unsigned *raw, const RowSpan &sp, int i)   // column sp.first + i, 0 <= i < sp.len
{
  const int b = sp.mis + i;
  return (raw[b >> 2] >> (8 * (b & 3))) & 0xffu;
}

// A member's workgroups share out the items of a row pass, a trip per workgroup: item = (nth job * rows + r) * nseg + g, from
// blockIdx.x - m->first in steps of m->nblk
struct RowItem { int nth, r, g; };   // the nth job (a source plane or a chain), its row, the segment of the row
__device__ __forceinline__ RowItem row_item(unsigned long long item, unsigned long long per_job, int nseg)
{
  return RowItem{(int)(item / per_job), (int)((item % per_job) / nseg), (int)(item % nseg)};
}

// A member's waves (`waves` per workgroup) share out the items of a column pass, a trip per wave: from first_wave_item by wave_item_step
__device__ __forceinline__ unsigned long long first_wave_item(const CvhIoMember *m, int waves)
{
  return (unsigned long long)(blockIdx.x - m->first) * waves + (threadIdx.x >> 6);
}
__device__ __forceinline__ unsigned long long wave_item_step(const CvhIoMember *m, int waves) { return (unsigned long long)m->nblk * waves; }

// item = band * nstrip + strip, bands of `rows` rows: the lane's rows r0 .. r1 - 1, its first column cc and how many of its four columns
// lie inside the plane (valid <= 0: none)
struct ColumnItem { int r0, r1, cc, valid; };
__device__ __forceinline__ ColumnItem column_item(unsigned long long item, int nstrip, int rows, int h, int w)
{
  const int r0 = (int)(item / nstrip) * rows, cc = (int)(item % nstrip) * kStrip + 4 * (int)(threadIdx.x & 63);
  return ColumnItem{r0, min(r0 + rows, h), cc, min(4, w - cc)};
}

static_assert(255ll * 4 * 65025 < (1ll << 32), "a lane's 32-bit plane sums hold one trip of the tallest band: cvh_rank_band_rows(127) = 255 rows");

}  // namespace
