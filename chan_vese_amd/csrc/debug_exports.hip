// debug_exports.hip — diagnostic exports that include/chanvese_hip.h does not declare (the tests and tools/ bind them by name).
#include "cvh_host.h"
#include "wave_math.h"
#include "local_math.h"
#include "smooth_math.h"
#include "rank_math.h"

// Diagnostic (not part of include/chanvese_hip.h): the strip table for a geometry, without a device.  out needs S + 1 ints.
extern "C" int cvh_debug_strip_bounds(int kind, int h, int tiles_x, int S, int strip_rows, int nblocks, int cls, int cskew, int skew, int *out)
{
  if (!out || S < 1 || h < 1 || (kind != 2 && kind != 3)) return CVH_ERR_ARG;
  std::vector<int> b;
  compute_strip_bounds(kind, h, tiles_x, S, strip_rows, nblocks, cls, cskew, skew, b);
  memcpy(out, b.data(), b.size() * sizeof(int));
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): which per-launch data flow resolve_geometry() picks for a shape and option set, without a
// device -- 0 tile kernel, 2 wave kernel, 3 wave kernel with 2 pixels per lane -- and its grid (tests/test_host_geometry.py pins the dispatch,
// e.g. the tile kernel from 2^28 pixels on, which no GPU test launches).
extern "C" int cvh_debug_data_flow(int h, int w, int channels, int math_mode, int kernel, int state_bits, int num_cus, int *flow, int *tiles_x,
                                   int *tiles_y, int *strip_rows)
{
  if (h < 1 || w < 1 || (channels != 1 && channels != 3) || !flow) return CVH_ERR_ARG;
  cvh_context c;
  c.h = h; c.w = w; c.C = channels; c.n = (size_t)h * (size_t)w;
  c.math_mode = math_mode; c.kernel = kernel; c.state_bits = state_bits; c.num_cus = num_cus > 0 ? num_cus : 256;
  const Geometry g = resolve_geometry(&c);
  *flow = g.strip;
  if (tiles_x) *tiles_x = g.tiles_x;
  if (tiles_y) *tiles_y = g.tiles_y;
  if (strip_rows) *strip_rows = g.strip_rows;
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): does the one-buffer flow of the 2-pixel kernel run (one_buffer_rule, csv_run.hip) for a
// shape and option set, without a device -- `live` = the co-resident contexts on the device (1: this one alone), `option` = "one_buffer".
extern "C" int cvh_debug_one_buffer(int h, int w, int channels, int math_mode, int kernel, int state_bits, int num_cus, int live, double tol,
                                    int option)
{
  if (h < 1 || w < 1 || (channels != 1 && channels != 3)) return -1;
  cvh_context c;
  c.h = h; c.w = w; c.C = channels; c.n = (size_t)h * (size_t)w;
  c.math_mode = math_mode; c.kernel = kernel; c.state_bits = state_bits; c.num_cus = num_cus > 0 ? num_cus : 256;
  c.p.tol = tol; c.one_buffer = option;
  return one_buffer_rule(&c, resolve_geometry(&c), live <= 1) ? 1 : 0;
}

// Diagnostic (not part of include/chanvese_hip.h): the one-buffer flow's shadow-row table (one_buffer_table, csv_run.hip) of a strip table
// b[0 .. S]; out needs S * 8 ints.
extern "C" int cvh_debug_one_buffer_table(const int *b, int S, int h, int *out)
{
  if (!b || !out || S < 1) return CVH_ERR_ARG;
  std::vector<int> tab;
  one_buffer_table(std::vector<int>(b, b + S + 1), h, tab);
  memcpy(out, tab.data(), tab.size() * sizeof(int));
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): the grid section and the work of ONE member of h x w pixels in a member-table kernel,
// without a device -- from the very functions the host units size a member's section with.  *items: the units the section's lanes, waves
// or workgroups share out; *nblk: its workgroups; *takers: how many units a workgroup takes per trip (CVH_BLOCK lanes, CVH_BLOCK / 64
// waves, or 1 where a workgroup owns a whole row or slot).  A unit i >= nblk * takers is taken on a second or later trip
// (tests/test_trip_counts.py pins the shapes of tests/test_gpu_second_trips.py to that).  For the two pyramid operations h x w is the FINE
// grid, as for cvh_restrict_blocks / cvh_prolong_blocks.
enum {
  TRIPS_IO = 0,          // ingest, image out, mask, histogram: 16-pixel pieces over lanes (the n % 16 last pixels go apart)
  TRIPS_START,           // threshold / rect / disk starts: pixel pairs over lanes (an odd last pixel goes apart)
  TRIPS_RESTRICT,        // 16 coarse pixels of a row, or the row's tail, over lanes
  TRIPS_PROLONG,         // two coarse pixels of a row over lanes
  TRIPS_ENERGY_TERMS,    // items (CVH_ENERGY_BAND rows x CVH_ENERGY_COLS columns) over waves
  TRIPS_ENERGY_REDUCE,   // item rows over the lanes of the member's one workgroup
  TRIPS_ROWS,            // reinit and score, row launch: rows over workgroups
  TRIPS_COLUMNS,         // reinit and score, column launches: band x 256-column slots, a workgroup each
  TRIPS_NOPS,            // = 8: the end of the ORIGINAL, contiguous codes -- no longer the number of operations
  // Codes added later start at 16 and 8 .. 15 stay refused for good (tests/test_trip_counts.py pins the first code behind the original
  // eight as refused): the enum has a permanent gap, the valid codes are 0 .. TRIPS_NOPS - 1 and TRIPS_MORPH_EMIT .. TRIPS_END - 1
  TRIPS_MORPH_EMIT = 16, // morphology and mask starts, emit launch: 16-pixel pieces over lanes (the n % 16 last pixels go apart)
  TRIPS_END
};

extern "C" int cvh_debug_trip_counts(int op, int h, int w, unsigned long long *items, unsigned *nblk, unsigned *takers)
{
  if (op < 0 || (op >= TRIPS_NOPS && op < TRIPS_MORPH_EMIT) || op >= TRIPS_END || h < 1 || w < 1 || !items || !nblk || !takers) return CVH_ERR_ARG;
  const size_t n = (size_t)h * (size_t)w;
  const unsigned bands = ((unsigned)h + CVH_REINIT_BAND - 1) / CVH_REINIT_BAND, chunks = ((unsigned)w + CVH_BLOCK - 1) / CVH_BLOCK;
  switch (op) {
    case TRIPS_IO: *items = n / 16; *nblk = cvh_io_blocks(n); *takers = CVH_BLOCK; break;
    case TRIPS_START: *items = n / 2; *nblk = cvh_init_start_blocks(n); *takers = CVH_BLOCK; break;
    case TRIPS_RESTRICT: *items = cvh_restrict_items(h, w); *nblk = cvh_restrict_blocks(h, w); *takers = CVH_BLOCK; break;
    case TRIPS_PROLONG: *items = cvh_prolong_items(h, w); *nblk = cvh_prolong_blocks(h, w); *takers = CVH_BLOCK; break;
    case TRIPS_ENERGY_TERMS: *items = cvh_energy_items(h, w); *nblk = cvh_energy_blocks(h, w); *takers = CVH_BLOCK / 64; break;
    case TRIPS_ENERGY_REDUCE: *items = cvh_energy_items(h, w); *nblk = 1; *takers = CVH_BLOCK; break;
    case TRIPS_ROWS: *items = (unsigned long long)h; *nblk = cvh_reinit_row_blocks(h); *takers = 1; break;
    case TRIPS_COLUMNS: *items = (unsigned long long)bands * chunks; *nblk = cvh_reinit_column_blocks(h, w); *takers = 1; break;
    case TRIPS_MORPH_EMIT: *items = n / 16; *nblk = cvh_io_blocks(n); *takers = CVH_BLOCK; break;
  }
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): the sections of a member of h x w pixels and `edges` boundary edges in the launches of
// cvh_contours*, from the functions contour_run.hip sizes them with.  *pixel_blocks: workgroups of the pixel launches, one count each;
// *scan_trip: counts the member's one-wave scan takes per trip; *edge_blocks: workgroups of the edge launches; *edge_lanes: edges (or
// pixels) their lanes cover per trip.
extern "C" int cvh_debug_contour_trips(int h, int w, unsigned long long edges, unsigned *pixel_blocks, unsigned *scan_trip, unsigned *edge_blocks,
                                       unsigned long long *edge_lanes)
{
  if (h < 1 || w < 1 || !pixel_blocks || !scan_trip || !edge_blocks || !edge_lanes) return CVH_ERR_ARG;
  *pixel_blocks = cvh_cc_blocks((size_t)h * (size_t)w);
  *scan_trip = cvh_contour_scan_trip();
  *edge_blocks = cvh_contour_edge_blocks((size_t)edges, (size_t)h * (size_t)w);
  *edge_lanes = (unsigned long long)*edge_blocks * CVH_BLOCK;
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): the tile grid of the resident flow (csv_resident_kernel.hip) for a plane of `channels`
// channels on `num_cus` CUs, one workgroup per CU, without a device -- the arithmetic resident_geometry() ends in.  Returns 1 and fills
// tiles_x, tiles_y and the rows of the tallest tile, or 0: the plane does not qualify (odd width, < 16 rows or columns, more rows per tile
// than the LDS of a CU holds for that channel count).  The options a context adds ("resident", FAST, chain-mode sums ...) are not part of it.
extern "C" int cvh_debug_resident_grid(int h, int w, int channels, int num_cus, int *tiles_x, int *tiles_y, int *tile_rows)
{
  if (h < 1 || w < 1 || num_cus < 1) return 0;
  ResidentGeom rg;
  if (!resident_tile_grid(h, w, channels, num_cus, num_cus, &rg)) return 0;
  if (tiles_x) *tiles_x = rg.tc;
  if (tiles_y) *tiles_y = rg.tr;
  if (tile_rows) *tile_rows = (h + rg.tr - 1) / rg.tr;
  return 1;
}

// Diagnostic (not part of include/chanvese_hip.h): the synchronisation words of the last resident launch: {error, 0, generation of
// the arrival line of tile 0 .. n-1, generation of the release line of tile 0 .. n-1}.
extern "C" int cvh_debug_resident_read(cvh_context *c, unsigned *out, int ngo)
{
  if (!c || !out || ngo < 0 || ngo > CVH_RESIDENT_MAX_TILES) return CVH_ERR_ARG;
  if (!c->d_resident) return fail(c, CVH_ERR_STATE, "no resident launch yet");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned> tmp(sizeof(CvhResident) / sizeof(unsigned));
  HIPCHK(c, hipMemcpy(tmp.data(), c->d_resident, sizeof(CvhResident), hipMemcpyDeviceToHost));
  out[0] = tmp[0]; out[1] = tmp[1] | (tmp[2] << 12) | (tmp[3] << 24);   // error; t_first | nit << 12 | steps_done as the kernel read it << 24
  for (int i = 0; i < ngo; ++i) { out[2 + i] = tmp[16 + (size_t)i * 16]; out[2 + ngo + i] = tmp[16 + (size_t)CVH_RESIDENT_MAX_TILES * 16 + (size_t)i * 16]; }
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): the h * w doubles the most recent Perona-Malik call of at least one time step on this
// context (its own cvh_perona_malik, or a cvh_perona_malik_batch it was a member of) left for its LAST channel -- the very plane pm_store rounded into
// that channel's uint8 plane (tests/test_gpu_pm_state.py holds every flow's doubles against the oracle's).  CVH_ERR_STATE before the
// first such call and after one that failed on the device; a call refused for its arguments leaves the previous plane in place.
extern "C" int cvh_debug_pm_plane(cvh_context *c, double *out)
{
  if (!c || !out) return CVH_ERR_ARG;
  if (c->pm_plane < 0 || c->pm_plane > 1 || !c->d_pm[c->pm_plane])
    return fail(c, CVH_ERR_STATE, "cvh_debug_pm_plane: no Perona-Malik call has left a plane on this context");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->d_pm[c->pm_plane], c->n * sizeof(double), hipMemcpyDeviceToHost));
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): the CUs of the context's device, what the automatic geometry and a fused batch's
// shares are sized for (tests/test_gpu_fused_batch_matrix.py recomputes a member's share geometry from it).
extern "C" int cvh_debug_num_cus(cvh_context *c, int *out)
{
  if (!c || !out) return CVH_ERR_ARG;
  *out = c->num_cus;
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): launch sets of cvh_reinit / cvh_reinit_batch so far in this process -- one set is the
// three kernels of reinit_kernels.hip over all members of the call (tests/test_gpu_reinit.py: a batch of n is one set, not n).
extern "C" unsigned long cvh_debug_reinit_launch_sets(void) { return g_launches[kReinitLaunchSets].load(); }
extern "C" unsigned long cvh_debug_pyramid_launches(void) { return g_launches[kPyramidLaunches].load(); }
// Diagnostics (not part of include/chanvese_hip.h): launches of cvh_convert_colour* / cvh_luma_image* so far in this process (a batch of n
// is one), and the pixels a workgroup of colour_kernels.hip takes per trip (tests/colour_util.py sizes a plane of one workgroup + one piece)
extern "C" unsigned long cvh_debug_colour_launches(void) { return g_launches[kColourLaunches].load(); }
extern "C" int cvh_debug_colour_block_pixels(void) { return CVH_COLOUR_BLOCK_PIXELS; }
// Diagnostics (not part of include/chanvese_hip.h) of cvh_local_planes*: launch sets so far in this process (a batch of n pairs is one:
// the row pass, where a pair takes a mean or a deviation, and the column pass); the windowed passes' geometry (CVH_WINDOW_*), from which
// tests/local_util.py derives the seam shapes -- out[0] rows of a band, out[1] columns of a strip, out[2] columns of a row segment --;
// and the per-pixel arithmetic of local_math.h compiled for the host: the floor square root (q <= 65025), and MEAN and DEV of a
// window of n pixels with sum S and sum of squares Q (tests/test_local_restatement.py holds both against Python integers)
extern "C" unsigned long cvh_debug_local_launch_sets(void) { return g_launches[kLocalLaunchSets].load(); }
extern "C" void cvh_debug_local_geometry(int *out) { out[0] = CVH_WINDOW_BAND; out[1] = CVH_WINDOW_STRIP; out[2] = CVH_WINDOW_SEGMENT; }
extern "C" unsigned cvh_debug_local_isqrt(unsigned q) { return cvh_local_isqrt(q); }
extern "C" void cvh_debug_local_stats(unsigned n, unsigned S, unsigned Q, unsigned *mean, unsigned *dev)
{
  *mean = cvh_local_mean(n, S);
  *dev = cvh_local_dev(n, S, Q);
}
// Diagnostics (not part of include/chanvese_hip.h) of cvh_rank_planes*: launch sets so far in this process (a batch of n pairs is one: up to
// five launches); the same geometry and the median's, from which tests/rank_util.py derives the seam shapes -- out[0] rows of a column band
// at R = 0 (at radius R: cvh_debug_rank_band_rows), out[1] columns of a strip, out[2] columns of a row segment, out[3] rows and out[4]
// columns of a median trip --; and the integer arithmetic of rank_math.h compiled for the host: a code's chain and whether it runs twice,
// the rows of a band at a radius, the rank of the lower median, and the walk over sixteen packed byte counters
extern "C" unsigned long cvh_debug_rank_launch_sets(void) { return g_launches[kRankLaunchSets].load(); }
extern "C" void cvh_debug_rank_geometry(int *out)
{
  out[0] = CVH_WINDOW_BAND; out[1] = CVH_WINDOW_STRIP; out[2] = CVH_WINDOW_SEGMENT; out[3] = CVH_RANK_MEDIAN_BAND; out[4] = CVH_RANK_MEDIAN_STRIP;
}
extern "C" int cvh_debug_rank_chain(int code) { return cvh_rank_chain(code); }
extern "C" int cvh_debug_rank_twice(int code) { return cvh_rank_twice(code); }
extern "C" int cvh_debug_rank_band_rows(int R) { return cvh_rank_band_rows(R, CVH_WINDOW_BAND); }
extern "C" unsigned cvh_debug_rank_median_index(unsigned n) { return cvh_rank_median_index(n); }
extern "C" int cvh_debug_rank_walk(const unsigned *words, unsigned *before, unsigned t) { return cvh_rank_walk(words, before, t); }
// Diagnostics (not part of include/chanvese_hip.h) of cvh_smooth_planes*: launch sets so far in this process (a batch of n pairs is one: the
// row pass, where a pair takes a blur or a detail plane, and the column pass); the passes' geometry at a radius, from which
// tests/smooth_util.py derives the seam shapes -- *band rows x *strip columns a workgroup of the column pass takes per trip, *segment
// columns of a row segment --; and the roundings of smooth_math.h compiled for the host (tests/test_smooth_restatement.py)
extern "C" unsigned long cvh_debug_smooth_launch_sets(void) { return g_launches[kSmoothLaunchSets].load(); }
extern "C" void cvh_debug_smooth_geometry(int radius, int *band, int *strip, int *segment)
{
  *band = cvh_smooth_band_rows(radius); *strip = CVH_SMOOTH_STRIP; *segment = CVH_WINDOW_SEGMENT;
}
extern "C" unsigned cvh_debug_smooth_row(unsigned a) { return cvh_smooth_row(a); }
extern "C" unsigned cvh_debug_smooth_blur(unsigned b) { return cvh_smooth_blur(b); }
extern "C" unsigned cvh_debug_smooth_detail(unsigned p, unsigned blur) { return cvh_smooth_detail(p, blur); }
// Diagnostic (not part of include/chanvese_hip.h): launch sets of cvh_energy / cvh_energy_batch so far in this process -- one set is the
// term pass and the reduce pass of energy_kernels.hip over all members of the call (tests/test_gpu_energy.py: a batch of n is one set)
extern "C" unsigned long cvh_debug_energy_launch_sets(void) { return g_launches[kEnergyLaunchSets].load(); }
// Diagnostic (not part of include/chanvese_hip.h): launch sets of cvh_score_mask* so far in this process -- one set is the four launches of
// score_kernels.hip over all members of the call (tests/test_gpu_score.py: a batch of n is one set)
extern "C" unsigned long cvh_debug_score_launch_sets(void) { return g_launches[kScoreLaunchSets].load(); }
// Diagnostic (not part of include/chanvese_hip.h): launch sets of cvh_get_mask_morph* / cvh_morph_levelset* / cvh_init_mask* so far in this
// process -- one set is every launch of morph_kernels.hip (and of the cleaning) over all members of the call (tests/test_gpu_morph.py: a
// batch of n is one set)
extern "C" unsigned long cvh_debug_morph_launch_sets(void) { return g_launches[kMorphLaunchSets].load(); }
// Diagnostic (not part of include/chanvese_hip.h): calls of cvh_split* / cvh_split_levelset* so far in this process (a batch of n is one), and
// the growth sweeps that ran in them -- a sweep that returned at once behind a sweep without changes is not counted, the sweep that found
// no change is (tests/test_gpu_split.py: the spiral takes more sweeps than a group holds)
extern "C" unsigned long cvh_debug_split_launch_sets(void) { return g_launches[kSplitLaunchSets].load(); }
extern "C" unsigned long cvh_debug_split_sweeps(void) { return g_launches[kSplitSweeps].load(); }
// Diagnostic (not part of include/chanvese_hip.h): pair launches of cvh_overlaps* so far in this process -- one per call for all its
// members, and one more each time a member's table overflowed and grew (tests/test_gpu_overlap.py: a table of 9216 pairs grows)
extern "C" unsigned long cvh_debug_overlap_launch_sets(void) { return g_launches[kOverlapLaunchSets].load(); }

// Diagnostic (not part of include/chanvese_hip.h): device time (HIP events on the leader's stream: table copy, the three launches, flag
// copy) of the last cvh_reinit / cvh_reinit_batch this context led (tools/reinit_probe.py).
extern "C" int cvh_debug_last_reinit_ms(cvh_context *c, float *ms)
{
  if (!c || !ms) return CVH_ERR_ARG;
  *ms = c->last_reinit_ms;
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): copies the stamp buffer of "debug_times".
extern "C" int cvh_debug_read(cvh_context *c, unsigned long long *out, long max_words, long *words, int *nblocks)
{
  if (!c || !out || !words) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  long n = (long)c->dbg_words < max_words ? (long)c->dbg_words : max_words;
  *words = n;
  if (nblocks) *nblocks = c->last_nparts > 0 ? c->last_nparts : resolve_geometry(c).nblocks;   // the grid the stamps belong to (a fused batch's share)
  if (n > 0 && c->d_dbg) HIPCHK(c, hipMemcpy(out, c->d_dbg, (size_t)n * 8, hipMemcpyDeviceToHost));
  return CVH_OK;
}

// Diagnostic (not part of include/chanvese_hip.h): the FAST flavour's per-pixel arithmetic on a vector of arguments, through the very
// inline functions the step kernels call (wave_math.h, csv_device.h) with the tables api.hip fills and the far-field series csv_run.hip
// sets up (tests/test_gpu_csv_math.py holds them against tests/golden/csv_math_ref.npz).  Ops (x holds cvh_debug_csv_math_arity(op)
// vectors of n, one after the other):
enum {
  MATH_H_FAR = 0,       // heaviside_centred_far(x) (clamped below 32 eps)
  MATH_H_NEAR,          // heaviside_centred_near(x), table staged in LDS
  MATH_H_FAST,          // far + near_field_correction: what a FAST wave / resident kernel's sums carry for a pixel
  MATH_H_STRICT,        // heaviside_strict(x)
  MATH_ATAN_TABLE,      // atan_table(x) (eps unused)
  MATH_INV_DELTA,       // inv_delta_eps: 1/delta_eps(x), wave / resident kernels
  MATH_DELTA,           // rcp_refined(inv_delta_eps(x))
  MATH_INV_DELTA_TILE,  // inv_delta_eps_tile: 1/delta_eps(x), tile kernel
  MATH_DELTA_TILE,      // rcp_refined(inv_delta_eps_tile(x))
  MATH_RCP,             // rcp_refined(x)
  MATH_RSQRT,           // rsqrt_refined(x)
  MATH_NORMALISED,      // normalised<true>(x0, x1)
  MATH_NORMALISED4,     // normalised4(x0, x1, x2)
  MATH_NOPS
};

extern "C" int cvh_debug_csv_math_arity(int op)
{
  return op < 0 || op >= MATH_NOPS ? 0 : op == MATH_NORMALISED ? 2 : op == MATH_NORMALISED4 ? 3 : 1;
}

namespace {
constexpr int kMathTab = 2 * CVH_ATAN_N + CVH_ATAN2_N;

__global__ void __launch_bounds__(256) csv_math_kernel(int op, int n, const double *x, double eps, double inv_eps, double dk1, double dk2,
                                                       cvh_dev::FarCoef fc, const double *tab, double *out)
{
  using namespace cvh_dev;
  __shared__ double stab[kMathTab];   // [0, 2 CVH_ATAN_N): atan_table's; then heaviside_centred_near's, as the kernels stage them
  for (int q = threadIdx.x; q < kMathTab; q += blockDim.x) stab[q] = tab[q];
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  const double *satan2 = stab + 2 * CVH_ATAN_N;
  double r = 0.0;
  switch (op) {
    case MATH_H_FAR: r = heaviside_centred_far(v, fc); break;
    case MATH_H_NEAR: r = heaviside_centred_near(v, inv_eps, satan2); break;
    case MATH_H_FAST: r = heaviside_centred_far(v, fc) + near_field_correction(v, inv_eps, satan2, fc); break;
    case MATH_H_STRICT: r = heaviside_strict(v, eps); break;
    case MATH_ATAN_TABLE: r = atan_table(v, stab); break;
    case MATH_INV_DELTA: r = inv_delta_eps(v, eps * eps, dk1); break;
    case MATH_DELTA: r = rcp_refined(inv_delta_eps(v, eps * eps, dk1)); break;
    case MATH_INV_DELTA_TILE: r = inv_delta_eps_tile(v, dk1, dk2); break;
    case MATH_DELTA_TILE: r = rcp_refined(inv_delta_eps_tile(v, dk1, dk2)); break;
    case MATH_RCP: r = rcp_refined(v); break;
    case MATH_RSQRT: r = rsqrt_refined(v); break;
    case MATH_NORMALISED: r = normalised<true>(v, x[(size_t)n + i]); break;
    case MATH_NORMALISED4: r = normalised4(v, x[(size_t)n + i], x[2 * (size_t)n + i]); break;
  }
  out[i] = r;
}
}  // namespace

extern "C" int cvh_debug_csv_math(int op, int n, const double *x, double eps, double *out)
{
  const int arity = cvh_debug_csv_math_arity(op);
  if (!arity || n < 1 || !x || !out || !(eps > 0)) return CVH_ERR_ARG;
  double tab[kMathTab];
  fill_atan_tables(tab);
  cvh_dev::FarCoef fc;
  {
    double k[5];
    far_coef(eps, 5, k, &fc.thr);
    fc.k0 = k[0]; fc.k1 = k[1]; fc.k2 = k[2]; fc.k3 = k[3]; fc.k4 = k[4];
  }
  const double pi = 3.14159265358979323846;   // as fill_args() derives inv_eps, dk1, dk2
  double *d_x = nullptr, *d_out = nullptr, *d_tab = nullptr;
  const size_t xbytes = (size_t)arity * (size_t)n * sizeof(double), obytes = (size_t)n * sizeof(double);
  hipError_t e = hipMalloc((void **)&d_x, xbytes);
  if (e == hipSuccess) e = hipMalloc((void **)&d_out, obytes);
  if (e == hipSuccess) e = hipMalloc((void **)&d_tab, sizeof(tab));
  if (e == hipSuccess) e = hipMemcpy(d_x, x, xbytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_tab, tab, sizeof(tab), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(csv_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, n, d_x, eps, 1.0 / eps, pi / eps, pi * eps, fc, d_tab, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, obytes, hipMemcpyDeviceToHost);
  hipFree(d_x); hipFree(d_out); hipFree(d_tab);
  if (e != hipSuccess) return fail(nullptr, CVH_ERR_HIP, "cvh_debug_csv_math: HIP error %d (%s)", (int)e, hipGetErrorString(e));
  return CVH_OK;
}
