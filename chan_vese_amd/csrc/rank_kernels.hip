// rank_kernels.hip — rank and grey-morphology planes on the device (gfx950): plane k of a member is COPY, MIN, MAX, MEDIAN, OPEN, CLOSE,
// TOPHAT or BOTHAT of a plane of its source context over the (2 R + 1)^2 window truncated at the border (include/chanvese_hip.h, "Rank
// planes").  Batch kernels over io_run.hip's member table like local_kernels.hip's: ONE grid serves N members of any mix of shapes, channel
// counts, radii and codes, a member owning the workgroups first .. first + nblk - 1; every launch reads the same table.  The passes'
// geometry, the staging of a row span and the sharing out of items are window_device.h's; here are the arithmetic and the writer.
// MIN and MAX are separable, and by van Herk / Gil-Werman the work per pixel does not grow with R: with the row (or column) padded by R
// neutral entries on either side -- which IS the truncated window -- and cut into blocks of K = 2 R + 1, g the running minimum from a
// block's start and hh the one back from its end, the window of K entries that starts at padded position x is min(hh[x], g[x + 2 R]).  A
// maximum is the minimum of the inverted bytes; the kernels only ever take minima of bytes that are inverted where they are read or
// written.  A member's workspace (the destination's) holds, per source plane s it reads, CVH_RANK_SLOTS byte planes, rows
// cvh_window_pitch(w) apart: for chain c (0 begins with an erosion, 1 with a dilation; rank_math.h) 3 c + 0 the row pass's result T, 3 c + 1
// the eroded / dilated plane E, 3 c + 2 the column passes' hh; 6 the median M.
//   row pass      rank_rows_kernel, once for the first half of a chain (from the source plane) and once for the second (from E).  Of
//                 the staged span a lane scans kRowLane consecutive entries, a segmented wave scan and a carry across the four waves
//                 make g and hh of the span in LDS, and a lane writes four results as one word of T.
//   column pass   column_min: a band is cvh_rank_band_rows(R) rows, a lane's four adjacent columns one word.  The band starts on a
//                 block seam.  The lane marches up its band once for hh, which it writes to the workspace and alone reads again, then
//                 down with g in registers.  rank_columns_kernel writes E, for the chains that run twice; rank_final_kernel is the last
//                 column pass of every chain AND the writer: it subtracts for the hats (the source plane is read there), copies the
//                 COPY planes and the median, and writes the member's planes.
//   median        rank_median_kernel, R = 1 .. 7: a lane marches down a column with a private histogram of 256 byte counters in LDS, four
//                 bins per word, word (bin / 4) * 64 + lane, and sixteen coarse counters behind them: no two lanes share a word.  It adds
//                 the 2 R + 1 bytes of the row entering and removes those of the row leaving (clipped), and finds the bin of rank
//                 (n - 1) / 2 by a coarse and a fine walk of sixteen counters each (rank_math.h); n follows the truncated window.
// The source is only read.  No kernel waits for another workgroup; the launches follow each other on the stream.
#include "window_device.h"
#include "rank_math.h"

namespace {

constexpr int kMedianBlock = 128, kHistWords = 64 + 4;            // threads of a median workgroup; a lane's fine and coarse words
static_assert(kSegment == 4 * CVH_BLOCK, "a lane of the row pass writes four results");
static_assert(CVH_RANK_MEDIAN_RADIUS_MAX == 7 && 15 * 15 < 256, "a window's samples fit a byte counter");

__device__ __forceinline__ int what_of(const CvhIoMember *m, int k) { return (m->interleaved >> (3 * k)) & 7; }

// what the member's planes ask of chain c of source plane s: bit 0 its first half alone (MIN, MAX), bit 1 both halves
__device__ __forceinline__ unsigned use_of(const CvhIoMember *m, int s, int c)
{
  unsigned u = 0;
  for (int k = 0; k < m->C; ++k)
    if (source_of(m, k) == s && cvh_rank_chain(what_of(m, k)) == c) u |= cvh_rank_twice(what_of(m, k)) ? 2u : 1u;
  return u;
}

__device__ __forceinline__ gbytes_out slot_of(const CvhIoMember *m, int s, int which)
{
  return (gbytes_out)m->dst + (size_t)(s * CVH_RANK_SLOTS + which) * cvh_rank_slot_bytes(m->h, m->w);
}

__global__ void __launch_bounds__(CVH_BLOCK) rank_rows_kernel(const CvhIoMember *tab, int nmem, int second)
{
  __shared__ unsigned raw[kRawWords];
  __shared__ uint8_t fwd[kRowLane * CVH_BLOCK], bwd[kRowLane * CVH_BLOCK];
  __shared__ unsigned wave_total[2][CVH_BLOCK / 64];
  const CvhIoMember *m = tab + io_member(tab, nmem);
  unsigned jobs = 0;   // bit 2 s + c: chain c of source plane s takes this pass
  for (int s = 0; s < CVH_MAX_CHANNELS; ++s)
    for (int c = 0; c < 2; ++c) {
      const unsigned u = use_of(m, s, c);
      if (second ? (u & 2u) != 0 : u != 0) jobs |= 1u << (2 * s + c);
    }
  if (!jobs) return;   // (the whole workgroup)
  const int h = m->h, w = m->w, R = m->h2, K = 2 * R + 1;
  const int nseg = (w + kSegment - 1) / kSegment;
  const size_t pitch = cvh_window_pitch(w);
  const unsigned long long per_job = (unsigned long long)h * nseg, items = per_job * __popc(jobs);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (unsigned long long item = blockIdx.x - m->first; item < items; item += m->nblk) {
    const RowItem it = row_item(item, per_job, nseg);
    const int r = it.r, job = nth_set_bit<2 * CVH_MAX_CHANNELS>(jobs, it.nth), s = job >> 1, c = job & 1;
    // the first half of chain 1 and the second half of chain 0 are dilations: their bytes are inverted as they are read
    const unsigned flip = ((c != 0) != (second != 0)) ? 0xffffffffu : 0u;
    const gbytes_in in = second ? (gbytes_in)slot_of(m, s, 3 * c + 1) : (gbytes_in)m->src + (size_t)s * m->src_stride;
    const size_t stride = second ? pitch : (size_t)w;
    const int c0 = it.g * kSegment, cend = min(c0 + kSegment, w);
    const int span = cend - c0 + 2 * R;   // padded entries: entry i is column c0 + i - R, neutral outside the plane
    const RowSpan sp = stage_row_span(raw, in, r, stride, c0, cend, R, w, flip);
    auto entry = [&](int i) -> unsigned {
      const int x = c0 + i - R;
      return x < sp.first || x > sp.last ? 255u : span_byte(raw, sp, x - sp.first);
    };
    // g (back == false) or hh (back == true) of the span: a lane scans its kRowLane entries in scan order, restarting where a block
    // starts; a segmented scan over the lanes' (minimum, restarted) pairs gives every lane what lies in front of it in its block
    auto scan = [&](bool back, uint8_t *out) {
      unsigned loc[kRowLane], run = 255u, restarted = 0;   // bit j: a block started at or before entry j of this lane
      bool began = false;
#pragma unroll
      for (int j = 0; j < kRowLane; ++j) {
        const int e = kRowLane * tid + j, i = back ? span - 1 - e : e;
        unsigned v = 255u;
        bool start = false;
        if (e < span) {
          const int pos_mod = (c0 + i) % K;
          start = back ? pos_mod == K - 1 : pos_mod == 0;
          v = entry(i);
        }
        run = start ? v : min(run, v);
        began |= start;
        if (began) restarted |= 1u << j;
        loc[j] = run;
      }
      unsigned v = run, f = restarted != 0;
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned pv = __shfl_up(v, off, 64), pf = __shfl_up(f, off, 64);
        if (lane >= off) { if (!f) v = min(v, pv); f |= pf; }
      }
      if (lane == 63) wave_total[back ? 1 : 0][wave] = v | (f << 8);
      unsigned ev = __shfl_up(v, 1, 64), ef = __shfl_up(f, 1, 64);
      if (lane == 0) { ev = 255u; ef = 0; }
      __syncthreads();
      unsigned cv = 255u;   // what the waves in front hand over
      for (int u = 0; u < wave; ++u) {
        const unsigned t = wave_total[back ? 1 : 0][u];
        cv = (t >> 8) ? (t & 0xffu) : min(cv, t & 0xffu);
      }
      const unsigned carry = ef ? ev : min(cv, ev);
#pragma unroll
      for (int j = 0; j < kRowLane; ++j) {
        const int e = kRowLane * tid + j;
        if (e < span) out[back ? span - 1 - e : e] = (uint8_t)(((restarted >> j) & 1u) ? loc[j] : min(carry, loc[j]));
      }
    };
    scan(false, fwd);
    scan(true, bwd);
    __syncthreads();
    if (c0 + 4 * tid < cend) {   // four results as one aligned word of T; what lies behind column w - 1 stays inside the row's pitch
      unsigned word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * tid + j;
        if (c0 + i < cend) word |= min((unsigned)bwd[i], (unsigned)fwd[i + 2 * R]) << (8 * j);
      }
      *(gwords_out)(slot_of(m, s, 3 * c) + (size_t)r * pitch + c0 + 4 * tid) = word;
    }
    __syncthreads();   // the next trip rewrites the staging
  }
}

struct Four { unsigned v[4]; };
__device__ __forceinline__ Four unpack(unsigned x) { return Four{{x & 0xffu, (x >> 8) & 0xffu, (x >> 16) & 0xffu, x >> 24}}; }
__device__ __forceinline__ unsigned pack(const Four &a) { return a.v[0] | (a.v[1] << 8) | (a.v[2] << 16) | (a.v[3] << 24); }
__device__ __forceinline__ void min_into(Four &a, unsigned x)
{
  const Four b = unpack(x);
#pragma unroll
  for (int j = 0; j < 4; ++j) a.v[j] = min(a.v[j], b.v[j]);
}

// The column minimum over rows max(r - R, 0) .. min(r + R, h - 1) of the byte plane T for the rows r0 .. r1 - 1 of a band that starts
// on a block seam (r0 a multiple of the band's rows, those a multiple of K), for the lane's word of four columns: T, H point at the
// lane's word in row 0, rows are `pw` words apart.  emit(r, word) receives the results in ascending rows.  H receives hh of the band's
// rows: written and read by this lane alone.
template <class Emit>
__device__ __forceinline__ void column_min(gwords_in T, gwords_out H, size_t pw, int h, int R, int rows, int r0, int r1, Emit emit)
{
  const int K = 2 * R + 1;
  const Four neutral = Four{{255u, 255u, 255u, 255u}};
  Four run = neutral;
  const int top = min(r0 + rows - 1, h - 1 + R);   // padded rows behind it are neutral: padded row y is row y - R
  int mod = top % K;
  for (int y = top; y >= r0; --y) {
    if (mod == K - 1) run = neutral;
    if (y - R >= 0) min_into(run, T[(size_t)(y - R) * pw]);   // (y - R <= h - 1 by `top`)
    if (y < r1) H[(size_t)y * pw] = pack(run);
    mod = mod == 0 ? K - 1 : mod - 1;
  }
  run = neutral;
  mod = 0;   // r0 is a block seam
  for (int y = r0; y <= r1 - 1 + 2 * R; ++y) {
    if (mod == 0) run = neutral;
    if (y - R >= 0 && y - R < h) min_into(run, T[(size_t)(y - R) * pw]);
    const int r = y - 2 * R;
    if (r >= r0) {
      Four out = run;
      min_into(out, H[(size_t)r * pw]);
      emit(r, pack(out));
    }
    mod = mod == K - 1 ? 0 : mod + 1;
  }
}

// E of the chains that run twice: the column pass of their first half
__global__ void __launch_bounds__(CVH_BLOCK) rank_columns_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const int h = m->h, w = m->w, R = m->h2, Cs = m->w2;
  const int rows = cvh_rank_band_rows(R, kBand);
  const int nstrip = (w + kStrip - 1) / kStrip, nband = (h + rows - 1) / rows;
  const size_t pw = cvh_window_pitch(w) / 4;
  const unsigned long long items = (unsigned long long)nband * nstrip;
  const unsigned long long nwaves = wave_item_step(m, CVH_BLOCK / 64);
  for (unsigned long long item = first_wave_item(m, CVH_BLOCK / 64); item < items; item += nwaves) {
    const ColumnItem it = column_item(item, nstrip, rows, h, w);
    const int r0 = it.r0, r1 = it.r1, cc = it.cc;
    if (it.valid <= 0) continue;
    for (int s = 0; s < Cs; ++s)
      for (int c = 0; c < 2; ++c) {
        if (!(use_of(m, s, c) & 2u)) continue;
        const unsigned flip = c ? 0xffffffffu : 0u;   // chain 1 dilated: back to plain bytes
        const gwords_out E = (gwords_out)slot_of(m, s, 3 * c + 1) + cc / 4;
        column_min((gwords_in)slot_of(m, s, 3 * c) + cc / 4, (gwords_out)slot_of(m, s, 3 * c + 2) + cc / 4, pw, h, R, rows, r0, r1,
                   [&](int r, unsigned v) { E[(size_t)r * pw] = v ^ flip; });
      }
  }
}

// the last column pass of every chain and the writer of every plane
__global__ void __launch_bounds__(CVH_BLOCK) rank_final_kernel(const CvhIoMember *tab, int nmem)
{
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const int h = m->h, w = m->w, R = m->h2, C = m->C, Cs = m->w2;
  const int rows = cvh_rank_band_rows(R, kBand);
  const int nstrip = (w + kStrip - 1) / kStrip, nband = (h + rows - 1) / rows;
  const size_t pw = cvh_window_pitch(w) / 4;
  const unsigned long long items = (unsigned long long)nband * nstrip;
  const unsigned long long nwaves = wave_item_step(m, CVH_BLOCK / 64);
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  for (unsigned long long item = first_wave_item(m, CVH_BLOCK / 64); item < items; item += nwaves) {
    const ColumnItem it = column_item(item, nstrip, rows, h, w);
    const int r0 = it.r0, r1 = it.r1, cc = it.cc, valid = it.valid;
    if (valid <= 0) continue;
    const unsigned keep = valid == 4 ? 0xffffffffu : (1u << (8 * valid)) - 1u;
    unsigned s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
    auto write = [&](int k, int r, unsigned v) {
      store_bytes((gbytes_out)m->plane[k] + (size_t)r * w + cc, v, valid);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const unsigned x = (v >> (8 * j)) & 0xffu; s1[k] += x; s2[k] += x * x; }
    };
    for (int s = 0; s < Cs; ++s) {
      const gbytes_in plane = (gbytes_in)m->src + (size_t)s * m->src_stride;
      unsigned copies = 0, medians = 0, of_chain[2] = {0, 0};   // the member's planes that come from source plane s (wave-uniform)
#pragma unroll
      for (int k = 0; k < CVH_MAX_CHANNELS; ++k)
        if (k < C && source_of(m, k) == s) {
          const int code = what_of(m, k), chain = cvh_rank_chain(code);
          if (chain >= 0) of_chain[chain] |= 1u << k;
          else if (code == CVH_RANK_MEDIAN && R > 0) medians |= 1u << k;
          else copies |= 1u << k;   // (the median at R = 0 is the pixel)
        }
      if (copies | medians) {
        const gwords_in M = (gwords_in)slot_of(m, s, 6) + cc / 4;
        for (int r = r0; r < r1; ++r) {
          const unsigned p = copies ? load_bytes(plane + (size_t)r * w + cc, valid) : 0u;
          const unsigned med = medians ? M[(size_t)r * pw] & keep : 0u;
#pragma unroll
          for (int k = 0; k < CVH_MAX_CHANNELS; ++k)
            if (((copies | medians) >> k) & 1u) write(k, r, ((medians >> k) & 1u) ? med : p);
        }
      }
      for (int c = 0; c < 2; ++c) {
        if (!of_chain[c]) continue;
        const unsigned use = use_of(m, s, c);
        const bool twice = (use & 2u) != 0;
        // the chain's last half is a dilation for chain 0 run twice and for chain 1 run once: back to plain bytes
        const unsigned flip = ((c != 0) != twice) ? 0xffffffffu : 0u;
        bool hats = false;
#pragma unroll
        for (int k = 0; k < CVH_MAX_CHANNELS; ++k)
          if ((of_chain[c] >> k) & 1u) hats |= what_of(m, k) >= CVH_RANK_TOPHAT;
        const gwords_in E = (gwords_in)slot_of(m, s, 3 * c + 1) + cc / 4;
        column_min((gwords_in)slot_of(m, s, 3 * c) + cc / 4, (gwords_out)slot_of(m, s, 3 * c + 2) + cc / 4, pw, h, R, rows, r0, r1,
                   [&](int r, unsigned raw) {
          const unsigned v = (raw ^ flip) & keep;
          const unsigned p = hats ? load_bytes(plane + (size_t)r * w + cc, valid) : 0u;
          const unsigned half = (twice && (use & 1u)) ? E[(size_t)r * pw] & keep : v;   // MIN / MAX beside a chain that runs twice
#pragma unroll
          for (int k = 0; k < CVH_MAX_CHANNELS; ++k)
            if ((of_chain[c] >> k) & 1u) {
              const int code = what_of(m, k);
              // OPEN <= p <= CLOSE in every byte, so the words subtract without a borrow between bytes
              write(k, r, code == CVH_RANK_TOPHAT ? p - v : code == CVH_RANK_BOTHAT ? v - p : cvh_rank_twice(code) ? v : half);
            }
        });
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) flush(acc + 2 * k, s1[k], s2[k]);
  }
  add_sums(acc, C, m->sums);
}

__global__ void __launch_bounds__(kMedianBlock) rank_median_kernel(const CvhIoMember *tab, int nmem)
{
  __shared__ unsigned hist[kMedianBlock / 64][kHistWords * 64];
  const CvhIoMember *m = tab + io_member(tab, nmem);
  const int h = m->h, w = m->w, R = m->h2;
  unsigned need = 0;   // bit s: a MEDIAN plane of the member reads plane s of the source
  for (int k = 0; k < m->C; ++k)
    if (what_of(m, k) == CVH_RANK_MEDIAN) need |= 1u << source_of(m, k);
  if (!need || R == 0) return;
  const int nstrip = (w + 63) / 64, nband = (h + CVH_RANK_MEDIAN_BAND - 1) / CVH_RANK_MEDIAN_BAND;
  const size_t pitch = cvh_window_pitch(w);
  const unsigned long long per_plane = (unsigned long long)nband * nstrip, items = per_plane * __popc(need);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned *const mine = hist[wave] + lane;   // word q of this lane: mine[64 q]
  const unsigned long long nwaves = wave_item_step(m, kMedianBlock / 64);
  for (unsigned long long item = first_wave_item(m, kMedianBlock / 64); item < items; item += nwaves) {
    const int nth = (int)(item / per_plane), band = (int)((item % per_plane) / nstrip), col = (int)(item % nstrip) * 64 + lane;
    if (col >= w) continue;
    const int s = nth_set_bit<CVH_MAX_CHANNELS>(need, nth);   // the nth plane that is read
    const gbytes_in plane = (gbytes_in)m->src + (size_t)s * m->src_stride;
    const gbytes_out M = slot_of(m, s, 6);
    const int r0 = band * CVH_RANK_MEDIAN_BAND, r1 = min(r0 + CVH_RANK_MEDIAN_BAND, h);
    const int clo = max(col - R, 0), chi = min(col + R, w - 1);
    const unsigned nc = (unsigned)(chi - clo + 1);
    for (int q = 0; q < kHistWords; ++q) mine[64 * q] = 0;
    auto row = [&](int rr, bool enter) {   // the bytes of row rr in the window's columns enter or leave the histogram
      for (int j = clo; j <= chi; ++j) {
        const unsigned b = plane[(size_t)rr * w + j];
        const unsigned fine = 1u << (8 * (b & 3u)), coarse = 1u << (8 * ((b >> 4) & 3u));
        if (enter) { atomicAdd(&mine[64 * (b >> 2)], fine); atomicAdd(&mine[64 * (64 + (b >> 6))], coarse); }
        else { atomicSub(&mine[64 * (b >> 2)], fine); atomicSub(&mine[64 * (64 + (b >> 6))], coarse); }
      }
    };
    for (int rr = max(r0 - R, 0); rr <= min(r0 + R, h - 1); ++rr) row(rr, true);
    for (int r = r0; r < r1; ++r) {
      const unsigned nr = (unsigned)(min(r + R, h - 1) - max(r - R, 0) + 1), t = cvh_rank_median_index(nr * nc);
      unsigned words[4], before = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) words[q] = mine[64 * (64 + q)];
      const int g = cvh_rank_walk(words, &before, t) & 15;   // (one always exceeds: the counters hold nr * nc > t samples)
#pragma unroll
      for (int q = 0; q < 4; ++q) words[q] = mine[64 * (4 * g + q)];
      const int f = cvh_rank_walk(words, &before, t) & 15;
      M[(size_t)r * pitch + col] = (uint8_t)(16 * g + f);
      if (r + R + 1 <= h - 1) row(r + R + 1, true);
      if (r - R >= 0) row(r - R, false);
    }
  }
}

}  // namespace

// workgroups of a member: the largest of what the passes share out -- a trip per workgroup (rows of `row_jobs` chains) or per wave
// (columns; `median_planes` source planes of the median) --; the rest is taken on further trips
unsigned cvh_rank_blocks(int h, int w, int R, int row_jobs, int median_planes)
{
  const size_t band = (size_t)cvh_rank_band_rows(R, kBand);
  const size_t rows = (size_t)row_jobs * (size_t)h * (((size_t)w + kSegment - 1) / kSegment);
  const size_t cols = (((size_t)h + band - 1) / band) * (((size_t)w + kStrip - 1) / kStrip);
  const size_t meds = (size_t)median_planes * (((size_t)h + CVH_RANK_MEDIAN_BAND - 1) / CVH_RANK_MEDIAN_BAND) * (((size_t)w + 63) / 64);
  size_t b = (cols + CVH_BLOCK / 64 - 1) / (CVH_BLOCK / 64);
  if (rows > b) b = rows;
  if ((meds + kMedianBlock / 64 - 1) / (kMedianBlock / 64) > b) b = (meds + kMedianBlock / 64 - 1) / (kMedianBlock / 64);
  return (unsigned)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

hipError_t cvh_launch_rank(const CvhIoMember *tab, int nmem, unsigned grid, unsigned passes, hipStream_t s)
{
  if (passes & CVH_RANK_PASS_ROWS) hipLaunchKernelGGL(rank_rows_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem, 0);
  if (passes & CVH_RANK_PASS_TWICE) {
    hipLaunchKernelGGL(rank_columns_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
    hipLaunchKernelGGL(rank_rows_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem, 1);
  }
  if (passes & CVH_RANK_PASS_MEDIAN) hipLaunchKernelGGL(rank_median_kernel, dim3(grid), dim3(kMedianBlock), 0, s, tab, nmem);
  hipLaunchKernelGGL(rank_final_kernel, dim3(grid), dim3(CVH_BLOCK), 0, s, tab, nmem);
  return hipGetLastError();
}
