// cvh_host.h -- private header of the library's host units: the context, the launch geometries and the helpers more than one unit calls.
// api.hip (lifecycle, options, host-buffer I/O, getters, the transitions of a context's run state), csv_run.hip (CSV steps of one
// context), csv_batch.hip (fused batch, and what every batch shares: the member and pair checks, the member predicates, the grow-only
// device buffers), pm_run.hip (Perona-Malik), io_run.hip (device-memory I/O, reinitialisation, and the scaffolds of the member-table
// calls: MemberCall with its further waits, write_planes, the pointer checks, the launch counters), init_run.hip (device-side initial
// level sets), components_run.hip (connected components, and MaskSource: the raw or cleaned mask every mask-derived call starts from),
// pyramid_run.hip (coarse-to-fine), colour_run.hip (colour spaces), window_run.hip (local statistics, rank planes and smoothing: the windowed-plane calls), energy_run.hip (the functional's terms), score_run.hip (mask scores),
// morph_run.hip (mask morphology, mask starts), split_run.hip (object split), measure_run.hip (component measures), contour_run.hip (contours), overlap_run.hip
// (component overlaps), multiphase_run.hip (four phases: a pair of contexts iterated together), localized_run.hip (localised regions), geodesic_run.hip (edge-weighted length), convex_run.hip (convex relaxation), march_run.hip (the driver under those four; march_flow.h: their one call sequence, over each file's flow description), edge_run.hip (the edge plane), debug_exports.hip (diagnostics).  Kernel
// sources do not include it.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "cvh_internal.h"

// a grow-only device buffer of cap bytes: the tables of the batches a context leads (grow_table), and the buffers whose owner counts in
// elements -- rows, edges, points, slots -- and hands that count to its kernels (grow_table_to); free_table frees either
struct DeviceTable { void *d = nullptr; size_t cap = 0, count = 0; };

// One-buffer flow of the 2-pixel kernel: what option "one_buffer" starts as (DESIGN.md 4.1 holds the measurement that decides it), and the
// footprint the Infinity Cache holds reliably (tools/mall_sweep_probe.hip: at <= ~204 MB a ping-pong stream stays in the fast regime)
constexpr int CVH_ONE_BUFFER_DEFAULT = -1;
constexpr double kCachedFootprint = 205e6;
constexpr int kGraphSteps = 16;   // steps per captured graph (even: the ping-pong parity repeats)
struct StepGraph { hipGraphExec_t exec = nullptr; CvhStepArgs key[4]; int kind = -1, flavour = -1; };
struct BatchCache;   // the device tables of a fused batch whose first member this context is (cvh_enqueue_steps_batch)

struct cvh_context {   // opaque to callers; four groups
  // ---- identity and buffers: fixed by cvh_create, or allocated once on first use ----
  int h = 0, w = 0, C = 0, device = 0;
  size_t n = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  uint8_t *d_img[CVH_MAX_CHANNELS] = {nullptr, nullptr, nullptr};   // planes inside d_img_slab, img_stride bytes apart
  uint8_t *d_img_slab = nullptr;
  size_t img_stride = 0;
  double *d_u[2] = {nullptr, nullptr};
  void *d_u_slab = nullptr;
  float *d_uf[2] = {nullptr, nullptr};   // FP32 state (option "state"): what the iteration kernels read and write
  void *d_uf_slab = nullptr;
  CvhState *d_state = nullptr;
  CvhState *h_state = nullptr;  // pinned, four slots for pipelined polling
  int *h_status = nullptr;  // pinned + mapped: {steps_done, stopped} written by the device
  double *d_partials = nullptr;
  int partial_rows = 0;
  double *d_trace = nullptr;
  int trace_cap = 0;
  double *d_pm[2] = {nullptr, nullptr};
  int pm_plane = -1;            // which of d_pm[] pm_store read for the last channel of the most recent Perona-Malik call (-1: no call has
                                // stored a plane yet, or the last one failed on the device) -- cvh_debug_pm_plane; assigned in pm_run.hip
  uint8_t *d_mask = nullptr;
  double *d_dummy = nullptr;
  double *d_atan = nullptr;
  CvhChainAcc *d_chain = nullptr;   // chain mode of the 2-pixel wave kernel (cvh_internal.h, CvhChainAcc)
  int *d_bounds = nullptr;      // wave kernel: first row of every strip, [tiles_y + 1]
  std::vector<int> h_bounds;    // the table d_bounds holds (upload_strip_bounds)
  double *d_ob = nullptr;       // one-buffer flow: the padded slab (cvh_internal.h, cvh_ob_*), allocated on first use, grown on demand
  size_t ob_cap = 0;            // its bytes
  int *d_ob_tab = nullptr;      // and the strips' shadow-row table, [h][CVH_OB_TAB]
  unsigned long long *d_isums = nullptr, *h_isums = nullptr;   // image_sums_kernel (io_kernels.hip): {sum p, sum p^2} per plane (device / pinned)
  unsigned long long *d_dbg = nullptr;  // diagnostic stamps (option "debug_times")
  size_t dbg_words = 0;
  // resident kernel (csv_resident_kernel.hip): cache-resident planes iterate in LDS, one cooperative launch per chunk
  CvhResident *d_resident = nullptr;
  double *d_res_halo = nullptr;
  double *d_pm_halo = nullptr;   // pm_resident_kernel's border entries {value, tag}: its own buffer (tags must never meet foreign data)
  int *h_resident = nullptr;     // pinned: {arrive, error} of the last launch
  unsigned pm_res_serial = 0;    // launches of pm_resident_kernel so far (tag of the border entries; 0 = the cleared buffer)
  char err[512] = {0};
  // ---- run state: what the context has in flight and which of its cached values are still true.  Assigned by the transitions in
  // api.hip and by sync_impl, nowhere else -- but for the exceptions named at their field ----
  bool have_image = false, have_u = false, stop_valid = false;
  bool sums_valid = false;      // the state block holds c1 / c2 of the current level set (also cleared where eps or "state" change: api.hip)
  double sum_img[CVH_MAX_CHANNELS] = {0, 0, 0};
  double stop_norm = 0.0;  // || (sum_k I_k)/C ||_2
  // option "state" = 32 (declared FP32-state mode): the iteration kernels read and write d_uf[]; d_u[] stays the exchange format of
  // set / get / mask / contour / selection and of the initial sums -- a mirror, refreshed lazily (ensure_f64_mirror)
  bool mirror_valid = true;     // d_u[current] holds the level set (always true with 64-bit state)
  // one-buffer flow (csv_run.hip, one_buffer_flow): while ob_live the padded slab d_ob holds the level set and d_u[] is its mirror, refreshed
  // lazily like the FP32 state's (mirror_valid, ensure_f64_mirror).  Entered and left by one_buffer_flow / one_buffer_leave alone; a new
  // level set (levelset_arrived) lands in d_u[] and ends it.
  bool ob_live = false;
  int ob_key[6] = {0, 0, 0, 0, 0, 0};   // the strip table (bounds_key) and slab geometry the shadow rows were filled for
  int cur_base = 0;   // buffer that held u when the run counter was last reset
  int enqueued = 0;   // steps enqueued since then
  int steps_done = 0; // as of the last sync
  int chain_pb = 0;             // sum set that belongs to the level set at run-counter 0
  bool chain_pending = false;   // chain launches enqueued since the last flush
  bool chain_acc_valid = false; // the fixed-point sets hold the sums of the current level set
  int pending_nparts = 0;       // workgroup rows of sum u_diff^2 the pending iteration left (> 0: a per-launch wave kernel's, which the
                                // next launch on the same grid or the flush kernel books; 0: a resident launch's, booked inside it)
  int last_nparts = 0;          // workgroups (without the bookkeeper) of the last per-launch wave launch, own or fused (cvh_debug_read)
  bool resident_used = false;    // a resident launch since the last sync: its error word is checked there
  bool timing_open = false;     // ev0 is recorded and ev1 is not yet (the enqueue entry points open the interval, sync_impl closes it)
  // automatic cache policy of a run ("wave_pol" = -1): decided when the run's first iteration is enqueued, from the footprint of EVERY
  // context on this device that holds an image and a level set (live_footprint), and kept until the run counter is reset
  mutable int run_pol = -1;     // the decision of the current run (-1: not taken yet; taken in fill_args)
  mutable int run_alone = -1;   // 1: no other co-resident context on the device when the run started (automatic resident flow allowed; taken in run_is_alone)
  int run_chunk = -1;           // iterations of the enqueue at hand (cvh_enqueue_steps / cvh_warm: their argument; cvh_run: its chunk) -- how long a cooperative launch would be (-1: nothing announced yet; the enqueue entry points announce it)
  int geom_cus = 0;             // > 0: the CUs the automatic strip count is sized for (a fused batch: this context's share of the chip; batch_share)
  bool in_batch = false;        // a fused batch is preparing or enqueuing this member's launches (batch_share): they iterate the ping-pong pair
  double stop_cond_h = 0.0; // tol * stop_norm of the current run (a launch argument; prepare_host)
  float last_run_ms = 0.f, last_pm_ms = 0.f;
  float last_reinit_ms = 0.f;   // device interval (table copy, three launches, flag copy) of the last reinitialisation this context led
  // ---- options: cvh_set_params, cvh_set_option ----
  cvh_params p{};
  int state_bits = 64;          // option "state"
  int co_resident = 1;          // option "co_resident": 0 = a scratch / warm-up context that does not stream beside the others
  int math_mode = CVH_MATH_DEFAULT, finalize_mode = 0, sync_every = 32;
  int tile_rows = 0 /* auto */, use_lut = 1, use_dma = 0;
  int kernel = -1;      // -1 auto, 0 tile kernel, 2 wave kernel, 3 wave kernel with 2 pixels per lane
  int pm_kernel = -1;   // -1 auto (4 where the plane and the run qualify, else 3), 0 tile kernel, 1 wave kernel, 3 two time steps per launch, 4 resident plane
  int pm_strip_rows = 0;
  int wave_minw = 5, wave_lds_cap = 0, wave_prio = 1, wave_sync = -1 /* auto: 1 channel 1, 3 channels 0 */, wave_imgv = 1, wave_depth = 4;
  int res_prio = 1;     // option "res_prio": resident kernels, priority by quarters of a wave's band (csv_resident_kernel.hip)
  int res_go_share = 5;  // option "res_go_share": log2 of the tiles of an XCD that share one release line of the resident kernel (0: a line per tile, 5: a line per XCD, 6: one line)
  int one_buffer = CVH_ONE_BUFFER_DEFAULT;   // option "one_buffer": the 2-pixel kernel updates ONE padded level-set buffer in place (-1 auto by footprint, 0 off, 1 on wherever the flow exists)
  int wave_seam = 1;    // option "wave_seam": a strip's final group runs without prefetch and park in the 2-pixel kernel (csv_wave2_body.inc); 0 = with both
  int near_switch = 1;  // option "near_switch": per-wave, per-group choice of the form of H_eps (csv_wave2_kernel.hip); 0 = far form + correction always
  int wave_rev = 0, wave_xcd = 1;
  int use_graph = 1;
  int wave_skew = 0;            // per-mille: older workgroups get longer strips (see upload_strip_bounds)
  int chain_opt = 1;            // option "chain"
  int res_straight = 1;          // diagnostic option "res_straight": 0 = the generic march of csv_resident_kernel whatever the tile height
  int resident_opt = -1;         // option "resident": -1 auto (on where it applies, unless a per-launch knob was set), 0 off, 1 on where it applies
  int far_terms = 5;            // terms of the far-field series of H_eps (5: valid from 32 eps, 4: from 64 eps)
  int wave_pol = -1;            // option "wave_pol": cache policy of the 2-pixel kernel's rows (-1 auto by footprint, 0 plain, 1 write-through)
  int wave_cls = 1;             // 2-pixel wave kernel: class-major workgroup numbering (dispatch rounds)
  int wave_cskew = 500;         // per-mille strip-length skew between dispatch rounds (see upload_strip_bounds); measured
                                // in one process at 4096^2: 0 -> 61.1, 300 -> 59.3, 500 -> 58.7, 750 -> 58.5, 900 -> 59.2 us
  int strip_rows = 0;   // 0 auto
  int strips = 0;       // 2-pixel kernel: exact number of strips (0 auto); rows are dealt by cumulative weight, so any count works
  // ---- caches: graphs, tables, events and what was asked of the device once ----
  StepGraph graphs[4];          // by the chain-mode sum set of the first step, (chain_pb + enqueued) & 3; the ping-pong parity
                                // follows it (cur_base == chain_pb mod 2: levelset_arrived keeps that invariant)
  char pm_desc[256] = {0};      // what the last cvh_perona_malik launched (cvh_launch_info)
  hipGraphExec_t pm_graph = nullptr;   // 16 Perona-Malik steps starting from d_pm[0]
  CvhPmArgs pm_graph_key{};
  int pm_graph_kind = -1;
  int bounds_key[4] = {-1, -1, -1, -1};   // what d_bounds was computed for
  int tiles_x = 0, tiles_y = 0;
  BatchCache *batch = nullptr;  // fused batches led by this context: per-member launch arguments of the four phases, workgroup map
  DeviceTable pm_batch;          // Perona-Malik batches led by this context (cvh_perona_malik_batch): plane tables, workgroup maps
  // device-memory I/O led by this context (io_run.hip): the member table, sums and sine factors of a call on the device, their pinned
  // host image (also the landing place of sums and fetched planes), and the events that order a call against the caller's stream
  DeviceTable io_table;
  void *h_io = nullptr;
  size_t h_io_cap = 0;
  hipEvent_t ev_io_in = nullptr, ev_io_out = nullptr;   // ev_io_out also marks the last read of h_io by a copy still in flight
  void *d_reinit = nullptr;      // workspace of cvh_reinit (class words + the two distance fields, reinit_kernels.hip): allocated by the
                                 // first call, idle while CSV streams -- not part of live_footprint
  void *d_cc = nullptr;          // workspace of cvh_components* / cvh_get_mask_clean* (components_kernels.hip), and the rows of the last
  DeviceTable cc_table;          // table: allocated by the first call that needs them, kept -- not part of live_footprint either
  DeviceTable regions;           // the rows of this context's last cvh_measure* table (measure_run.hip): 128 bytes per row asked for, grown on demand, kept
  void *d_contour = nullptr;     // per-pixel workspace of cvh_contours* (contour_run.hip; 6 bytes per pixel): allocated by the first call, kept
  DeviceTable contour_edges;     // its per-edge workspace (45 bytes per edge of the largest call so far), grown on demand, kept
  DeviceTable contour_points;    // cvh_contours / cvh_contours_subpixel (host forms): the points on their way down (8 / 16 bytes per point asked for), grown on demand, kept
  unsigned *d_hist = nullptr;    // the 255 C + 1 counters of cvh_histogram* / cvh_otsu_threshold / cvh_init_otsu* (init_kernels.hip): allocated by
                                 // the first call, kept
  void *d_energy = nullptr;      // workspace of cvh_energy* (energy_run.hip): a CvhState for means taken beside the run's, then the item rows of
                                 // energy_kernels.hip: allocated by the first call, kept -- not part of live_footprint either
  void *d_score = nullptr;       // workspace of cvh_score_mask* (score_run.hip): class and surface words, the distance fields and the truth plane the
                                 // host form stages (5.5 bytes per pixel): allocated by the first call, kept -- not part of live_footprint either
  void *d_morph = nullptr;       // workspace of cvh_get_mask_morph* / cvh_morph_levelset* / cvh_init_mask (morph_run.hip): two planes of band words, the
                                 // 16-bit distance field and a byte plane (3.25 bytes per pixel): allocated by the first call, kept -- not part of live_footprint either
  void *d_split = nullptr;       // workspace of cvh_split* / cvh_split_levelset* (split_run.hip): the growth's 64-bit keys, 8 bytes per pixel of the plane
                                 // rounded up to whole tiles: allocated (and its padding cleared) by the first call, kept -- not part of
                                 // live_footprint either; the calls also take the morphology and the components workspaces
  void *d_local = nullptr;       // workspace of cvh_local_planes* (window_run.hip) as their DESTINATION: the row sums of the source planes it reads, a
                                 // slot of 6 bytes per pixel per plane of this context: allocated by the first call that takes a mean or a
                                 // deviation, kept -- not part of live_footprint either
  void *d_rank = nullptr;        // workspace of cvh_rank_planes* (window_run.hip) as their DESTINATION: CVH_RANK_SLOTS byte planes per plane of this context
                                 // (7 bytes per pixel and plane): allocated by the first call that takes anything but copies, kept -- not part
                                 // of live_footprint either
  void *d_smooth = nullptr;      // workspace of cvh_smooth_planes* (window_run.hip) as their DESTINATION: the row pass's 16-bit values, a slot of 2 bytes
                                 // per pixel per plane of this context: allocated by the first call that takes anything but copies, kept -- not
                                 // part of live_footprint either; a member of its own, since a workspace is sized by the family that allocated it
  DeviceTable overlap;           // cvh_overlaps* (overlap_run.hip): overlap.count slots of the pair table and overlap.count / 2 rows behind them (24 bytes
                                 // per slot), grown where a call's table overflows, kept; d_overlap_plane: the int32 plane the host form stages
  void *d_overlap_plane = nullptr;   // (4 bytes per pixel) -- allocated by the first call that needs them, not part of live_footprint either
  void *d_multiphase = nullptr;  // workspace of cvh_multiphase_* as their FIRST context (multiphase_run.hip): the pair's state block and the items'
                                 // partial sums: allocated by the first call, kept -- not part of live_footprint either
  DeviceTable mp_trace;          // and the trace rows of the longest cvh_multiphase_run so far that asked for them, grown on demand, kept
  void *d_localized = nullptr;   // workspace of cvh_localized_* (localized_run.hip): state block, the items' partial sums, the 1 + C planes of
                                 // horizontal window sums and the C planes of T_k: (8 + 12 C) bytes per pixel, allocated by the first call, kept
  DeviceTable loc_trace;         // and the trace rows of the longest cvh_localized_run so far that asked for them, grown on demand, kept
  uint16_t *d_gq = nullptr;      // the edge plane of "Edge-weighted length" (edge_run.hip): h w values 0 .. 32768, g = gq 2^-15; allocated by the first
  bool have_gq = false;          // call that sets it, kept until replaced; no image or level-set call touches it
  void *d_geodesic = nullptr;    // workspace of cvh_geodesic_run* (geodesic_run.hip): the state block and the items' partial sums: allocated by the
                                 // first call, kept -- not part of live_footprint either
  DeviceTable geo_trace;         // and the trace rows of the longest cvh_geodesic_run so far that asked for them, grown on demand, kept
  void *d_convex = nullptr;      // workspace of cvh_convex_run* (convex_run.hip): the state block, the items' partial sums and the relaxation state -- v and
                                 // two sets of vbar, qx, qy, 56 bytes per pixel: allocated by the first call, kept -- not part of live_footprint either
  bool have_convex = false;      // a call has completed: the workspace holds a relaxation state, convex_cur names the set that is current.  Assigned
  int convex_cur = 0;            // in convex_run.hip alone; no other call reads or clears them
  DeviceTable cvx_trace;         // and the trace rows of the longest cvh_convex_run so far that asked for them, grown on demand, kept
  DeviceTable march_table;       // four-phase / localised / geodesic / convex calls led by this context (march_run.hip): the members' argument records and their
  void *h_march = nullptr;       // state table; h_march: its pinned host image and the landing place of the states, h_march_cap bytes --
  size_t h_march_cap = 0;        // grown on demand, kept
  int coop_launch = -1;          // does the device launch cooperatively (-1: not asked yet; launches_cooperatively)
  int resident_cap = -1;         // workgroups of csv_resident_kernel the device holds at once (-1: not asked yet, 0: unavailable)
  int pm_resident_cap = -1;      // workgroups of pm_resident_kernel the device holds at once (-1: not asked yet)
  // events, all created by cvh_create
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evp[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_join = nullptr; // fused batch: joins this context's stream with the leader's
};

struct Geometry { int strip; int rows; int tiles_x, tiles_y, strip_rows, nblocks; };
// Resident mode (csv_resident_kernel.hip): the plane is cut into tr x tc tiles of <= 128 x 128 pixels, one workgroup per tile, all
// co-resident (one per CU), the level set stays in LDS for a chunk of iterations.  Applies to 1 channel (3 channels with "resident" = 1),
// FAST arithmetic, chain-mode sums, even widths, and planes that fit: tiles <= what the device holds, every tile 16 .. 128 rows (three
// channels: 16 .. 96).
struct ResidentGeom { int tr, tc, band; };

constexpr int kPmMaxPerLaunch = 1 << 16;   // time steps of one launch of the resident kernel
constexpr int kPmPollCap = 2000000;        // polls before a wait of the resident kernel gives up

#define HIPCHK(ctx, call)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail((ctx), CVH_ERR_HIP, "HIP error %d (%s) in %s", (int)e_, hipGetErrorString(e_), \
                  #call);                                                                      \
  } while (0)

// Helpers shared between the host units: hidden, so that only the C ABI and what it always exported leave the library.
#pragma GCC visibility push(hidden)
inline bool use_fast(const cvh_context *c)
{
  const int m = c->math_mode == CVH_MATH_DEFAULT ? CVH_MATH_FAST : c->math_mode;
  return m == CVH_MATH_FAST;
}

inline int current_buffer(const cvh_context *c) { return (c->cur_base + c->steps_done) & 1; }

constexpr size_t kErrLen = 512;
char *create_err();   // api.hip: the kErrLen bytes behind cvh_last_error(NULL) -- what failed outside a context, on the calling thread
int fail(cvh_context *ctx, int code, const char *fmt, ...);

// api.hip: live-context registry, image statistics
bool run_is_alone(const cvh_context *c);
double live_footprint(const cvh_context *c);
int image_stats(cvh_context *c, const uint8_t *const *host_planes);
double stop_norm_host(const std::vector<const uint8_t *> &planes, size_t n);
void fill_atan_tables(double *tab);

// api.hip: one function per event that moves a context's run state (the group of that name in cvh_context)
int settle(cvh_context *c);
int reset_run_impl(cvh_context *c);
hipError_t clear_run_device(cvh_context *c, hipStream_t s);   // the device's half of a new run, enqueued on s
int levelset_arrived(cvh_context *c, bool device_cleared = false);
void steps_enqueued(cvh_context *c, int n, int nparts, bool chain, bool resident);
void sums_taken(cvh_context *c, bool chain);
bool stop_norm_exact_on_device(const cvh_context *c);
void planes_changed(cvh_context *c);
void plane_sums_arrived(cvh_context *c, const unsigned long long *isums, const double *host_norm);
int adopt_f32_state(cvh_context *c);
int ensure_f64_mirror(cvh_context *c);

// csv_run.hip: geometry, launch arguments and the per-launch / graph / resident flows of one context
Geometry resolve_geometry(const cvh_context *c);
bool use_chain(const cvh_context *c, const Geometry &g);
bool launches_cooperatively(cvh_context *c);
bool resident_geometry(cvh_context *c, ResidentGeom *rg);
bool resident_tile_grid(int h, int w, int channels, int num_cus, int cap_blocks, ResidentGeom *rg);
void fill_args(const cvh_context *c, CvhStepArgs *a, int in_buf, int step);
void far_coef(double eps, int far_terms, double k[5], double *thr);
int prepare_host(cvh_context *c);
int prepare(cvh_context *c);
void compute_strip_bounds(int kind, int h, int tiles_x, int S, int strip_rows, int nblocks, int cls, int cskew, int skew, std::vector<int> &b);
int upload_strip_bounds(cvh_context *c, const Geometry &g);
bool one_buffer_rule(const cvh_context *c, const Geometry &g, bool alone);
bool wants_one_buffer(const cvh_context *c, const Geometry &g);
void one_buffer_table(const std::vector<int> &b, int h, std::vector<int> &tab);
int one_buffer_flow(cvh_context *c, const Geometry &g);
int one_buffer_leave(cvh_context *c);
int launch_one_step(cvh_context *c, int in_buf, int step, bool capturing = false, CvhLaunchNote *note = nullptr);
int flush_for_grid(cvh_context *c, int nparts);
int ensure_resident_buffers(cvh_context *c);
int launch_resident(cvh_context *c, const ResidentGeom &rg, int nsteps, CvhLaunchNote *note);
int sync_impl(cvh_context *c);

// csv_batch.hip: what every batch of contexts shares
void batch_cache_free(cvh_context *c);
int batch_fail(cvh_context *const *ctxs, int n, int code, const char *fmt, ...);
enum MemberNeeds { kMembersListed, kMembersWithImage, kMembersForCsv };
int members_check(cvh_context *const *ctxs, int n, const char *what, MemberNeeds needs);
int members_below(cvh_context *const *ctxs, int n, const char *what, int k, int only = -1);
int members_distances_fit(cvh_context *const *ctxs, int n, const char *what, int only = -1);
template <class T>   // int or long
int members_caps_fit(cvh_context *const *ctxs, int n, const char *what, const void *const *lists, const T *caps, const char *noun, const char *without,
                     int only = -1);
int members_have_images(cvh_context *const *ctxs, int n, const char *what);
int members_have_levelsets(cvh_context *const *ctxs, int n, const char *what, int only = -1);
int members_mirrors_fresh(cvh_context *const *ctxs, int n, const char *what, int first = 0, const char *noun = "member");
// the two lists of a call on pairs in the order its messages name them, their names and role words, and which one is written
struct PairRoles { cvh_context *const *first, *const *second; const char *first_name, *second_name, *first_role, *second_role; bool second_is_dst; };
int pairs_check(const PairRoles &p, int n, const char *what, std::vector<cvh_context *> *all, const std::function<int(int)> &rule,
                const std::function<int()> &args = nullptr);
int pair_sources_have_images(cvh_context *const *all, int n, const char *what, const char *role);
int join_into_leader(cvh_context *const *ctxs, int n, const int *member = nullptr);
int grow_table(cvh_context *c, DeviceTable *t, size_t bytes);
int grow_table_to(cvh_context *c, DeviceTable *t, size_t want, size_t count, size_t bytes);
void free_table(DeviceTable *t);

// io_run.hip: launches so far in this process (debug_exports.hip): the launch sets (three kernels for all members) of cvh_reinit*, the
// launches of cvh_restrict_image* / cvh_prolong_levelset*, those of cvh_convert_colour* / cvh_luma_image*, and the launch sets (term pass and
// reduce pass for all members) of cvh_energy*, the launch sets (four kernels for all members) of cvh_score_mask*, and the launch sets (every
// kernel of the call, for all members) of cvh_get_mask_morph* / cvh_morph_levelset* / cvh_init_mask*, and the pair launches of cvh_overlaps*
// (one per call, and one more each time a member's table had to grow), and the launch sets (every pass of the family for all pairs) of
// cvh_local_planes*, of cvh_rank_planes* and of cvh_smooth_planes* (window_run.hip: a Family names its counter), and the calls of cvh_split* / cvh_split_levelset*
// with the growth sweeps that ran in them (a sweep that returned at once is not counted)
enum LaunchCounter { kReinitLaunchSets, kPyramidLaunches, kColourLaunches, kEnergyLaunchSets, kScoreLaunchSets, kMorphLaunchSets, kOverlapLaunchSets, kLocalLaunchSets, kRankLaunchSets, kSmoothLaunchSets, kSplitLaunchSets, kSplitSweeps, kLaunchCounters };
extern std::atomic<unsigned long> g_launches[kLaunchCounters];

// io_run.hip: what every call on device memory or on a member table shares (the comments are at the definitions)
int pointer_check(cvh_context *const *ctxs, int n, int i, const void *p, const char *what);
int element_pointer_check(cvh_context *const *ctxs, int n, int i, const void *p, size_t size, const char *what);
int settle_all(cvh_context *const *ctxs, int n, const char *what);
int open_call(cvh_context *const *ctxs, int n, void *stream);
int close_call(cvh_context *const *ctxs, int n, void *stream, bool to_caller);
unsigned lay_out(CvhIoMember *tab, int n);
int mask_out(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, int invert, void *stream, const char *what);
void checkerboard_factors(int h, int w, double *out);   // api.hip: out[0 .. h-1] = sin(pi i/5), out[h .. h+w-1] = sin(pi j/5), host libm
void levelset_target(const cvh_context *c, CvhIoMember *m);
int ensure_workspace(cvh_context *c, void **slot, size_t bytes, const char *name, bool mirror = true);

// march_run.hip: what the four-phase, localised and geodesic flows share -- "iterate the level sets of N contexts on the leader's stream".
// march_flow.h runs the whole call over a flow's description: ready, prepare, open, classes, records, lay-out, one-or-upload, iterate, results
void fill_front_args(const cvh_context *c, CvhFrontArgs *f);
// alpha = dt mu, beta = dt / C, gamma = -dt nu, the lambdas and stop = tol * stop_norm of c's equation into a record's fields
void march_params(const cvh_context *c, double *alpha, double *beta, double *gamma, double *lambda1, double *lambda2, double *stop);
std::string member_prefix(int i);   // "member 3: ": what opens a batch's message about member i
// What every march call refuses for a member m[0 .. per-1] before anything is touched, in this order: "state" = 32, h * w >= 2^28, no
// image (need_images), no level set.  The message goes to lead[0] and opens with `who` ("" or "member 3: "); it names "the context"
// (per = 1) or "context a" / "context b" (per = 2)
int march_rules(cvh_context *const *lead, int nlead, cvh_context *const *m, int per, const char *what, const char *who, bool need_images);
void march_strip_geometry(int h, int w, int *cols, int *strip_rows, int *items);   // cvh_multiphase_geometry / cvh_geodesic_geometry
int state_down(cvh_context *a, const void *d_state, void *out, size_t bytes);   // on a's stream, through its pinned state slots; waits
// The leader's table of a call: *h is `host_bytes` of zeroed pinned memory whose first `dev_bytes` the caller uploads to *d.  Every call
// that uses it ends with a host wait on the leader's stream, so the pinned block is free when the next one begins.
int march_stage(cvh_context *lead, size_t dev_bytes, size_t host_bytes, unsigned char **h, unsigned char **d);
// One run of n members of `per` contexts each (1: a localised or geodesic member; 2: a four-phase pair A, B); ctxs is flat,
// [member][role], the leader is ctxs[0]; who(k) opens what a message says about context k ("", "context a: ", "member 3: ", ...).  Its
// one caller is march_run (march_flow.h), after the flow has checked the members; then
//   begin:   refuses a trace's bad arguments, settles max_steps;                 -- march_run makes the members and their workspaces ready --
//   open:    grows every member's own trace table to the rows wanted, stages the leader's table -- [n records of rec_size bytes][n state
//            slots of state_stride bytes, each beginning with a CvhMarchCount] -- and opens the call;
//                                                                               -- march_run fills the records (record, d_state, cur) --
//   upload:  the table goes up, ONCE per call;                                   -- march_run enqueues what the flow puts in front of t = 0 --
//   iterate: times the run, enqueues the leader's sync_every iterations at a time through step(parity) -- iteration t has parity t & 1 and
//            reads buffer (cur + t) & 1 of every context -- and copies the state table (own_state, if set) down behind each chunk: ONE copy and ONE wait per
//            chunk, whatever n; ends when every member has stopped or max_steps iterations are enqueued.  Then it brings every level set
//            into the buffer a new one lands in (at most ONE copy each, by the parity of the member's own steps_done), does the device's
//            half of a new run, copies the trace rows out, closes the call, waits, and books the level sets as arrived.  state(i) is
//            member i's state afterwards.
struct MarchRun {
  cvh_context *const *ctxs; int n, per; const char *what;
  std::function<std::string(int)> who;
  int max_steps = 0;
  double *const *traces = nullptr;
  int trace_rows = 0, *rows = nullptr;
  std::vector<int> trace_cap, row_width, cur;   // per member, per member, per context
  std::vector<double *> d_trace;                // per member: its own table, or null
  unsigned char *h_tab = nullptr, *d_tab = nullptr;
  size_t rec_size = 0, state_off = 0, state_stride = 0, dev_bytes = 0, land_off = 0;
  const void *own_state = nullptr;   // n == 1, launches by value: the member's own state block, which comes down in place of the table's slot
  std::function<int(int k, int done)> bake;   // set: iterate calls it for context k, whose member did `done` iterations, in place of the copy that
                                              // brings a level set into the buffer a new one lands in -- the flow writes that buffer itself

  int begin(int max_steps, double *const *traces, int trace_rows, int *rows);
  int open(const std::function<DeviceTable *(int)> &table_of, const std::function<int(int)> &width_of, size_t rec_size, size_t state_stride);
  void *record(int r) const { return h_tab + (size_t)r * rec_size; }
  const void *d_record(int r) const { return d_tab + (size_t)r * rec_size; }
  void *d_state(int i) const { return d_tab + state_off + (size_t)i * state_stride; }
  const void *state(int i) const { return h_tab + land_off + (size_t)i * state_stride; }
  int upload();
  int iterate(const std::function<int(int parity)> &step);
};

// the (channel count, math mode) classes of a march launch: members of one class share a kernel instantiation and a section of the table
constexpr int kMarchClasses = 4;
inline int march_class(const cvh_context *c) { return (c->C == 1 ? 0 : 2) + (use_fast(c) ? 1 : 0); }
struct MarchClass { int first = 0, n = 0, C = 1, fast = 0; unsigned grid = 0, grid2 = 0; };   // records first .. first + n - 1; the sums of their grids (march_flow.h)

// components_run.hip: the mask of every member that a call starts from -- raw, or cleaned as cvh_get_mask_clean* cleans it -- for the
// components calls there and for measure_run.hip, overlap_run.hip, contour_run.hip and morph_run.hip.  The first member table of such a
// call is the mask launches': the level set in src, the mask bytes in dst, the components workspace in plane[], a word per member in sums.
// need_cc: the caller's own launches take the components workspace even for a raw mask (the numbering launch of measure and overlap).
struct MemberCall;
struct MaskSource {
  int conn = 4, invert = 0;
  long min_area = 0, fill_holes = 0;
  int keep_largest = 0;

  bool drop() const { return min_area > 1; }   // (every component has a pixel)
  bool cleaned() const { return drop() || fill_holes || keep_largest; }
  // the member list and cvh_get_mask_clean*'s argument checks
  int check(cvh_context *const *ctxs, int n, const char *what) const;
  // every member has a level set and is settled; with need_cc or a cleaned mask it has its components workspace and a plane the 31-bit
  // indices cover, else a fresh FP64 mirror alone
  int ready(cvh_context *const *ctxs, int n, const char *what, bool need_cc) const;
  // member i's entry of the call's first table: dst and the device address of its word are the caller's
  void fill(MemberCall *call, int i, void *dst, unsigned long long *sums, bool need_cc) const;
  // the mask launches on the leader's stream: a cleaned mask's (the plain mask first where step 1, the drop, is off); of a raw mask
  // the plain mask with raw_too, nothing without (the caller's own launches read the level set)
  int launch(const MemberCall &call, bool raw_too) const;
};

// floor(sqrt(r2)), exactly: the rows and columns a disk D(r2) reaches (morph_run.hip, split_run.hip)
inline unsigned disk_root(uint32_t r2)
{
  unsigned long long r = (unsigned long long)sqrt((double)r2);
  while (r * r > r2) --r;
  while ((r + 1) * (r + 1) <= r2) ++r;
  return (unsigned)r;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

// One call on a member table (checked members, iterations in flight settled by the caller).  The leader's pinned block `hb` is
//   [table][second table, if asked for][extra_dev bytes at extra_off] -- dev_bytes, zeroed, uploaded to `db` by run() --
//   [extra_host bytes at host_off] -- host only: the landing place of what the launches copy back;
// extra_off and host_off are 256-byte aligned.  begin() stages once and fills n, h, w, C of every member; the caller fills the rest
// (both tables stay writable behind run(): the pinned block is this call's until the leader's next begin()).
struct MemberCall {
  cvh_context *const *ctxs = nullptr;
  int n = 0;
  const char *what = nullptr;
  cvh_context *lead = nullptr;
  unsigned char *hb = nullptr, *db = nullptr;
  CvhIoMember *tab = nullptr, *tab2 = nullptr;
  size_t extra_off = 0, host_off = 0, dev_bytes = 0;
  unsigned grid = 0, grid2 = 0;   // of tab / tab2: laid out by run()

  int begin(cvh_context *const *ctxs_, int n_, const char *what_, size_t extra_dev = 0, size_t extra_host = 0, bool two_tables = false);
  const CvhIoMember *dtab() const { return (const CvhIoMember *)db; }
  const CvhIoMember *dtab2() const { return (const CvhIoMember *)(db + ((unsigned char *)tab2 - hb)); }
  // the members begin the run their new level set opens (all, or those with which[i] != 0): the launch did the device's half
  int arrived(const int *which = nullptr) const;
  // a call with a further host wait: t (tab or tab2), which the caller has written again behind run(), goes up again; then, behind the
  // launches and copies the caller enqueues, what run() does behind its own
  int upload_again(const CvhIoMember *t) const;
  int wait_again(void *stream, bool to_caller) const;

  // The sections are laid out; the leader's stream is joined with the members' and the caller's; `first` (if any) is recorded; the
  // device image goes up; launches() enqueues the kernels and what they copy back on the leader's stream; the members' streams, and
  // with to_caller the caller's, wait for that; with `wait` the host does too -- the ONE host wait of such a call.
  template <class F>
  int run(void *stream, bool to_caller, bool wait, F launches, hipEvent_t first = nullptr)
  {
    grid = lay_out(tab, n);
    if (tab2) grid2 = lay_out(tab2, n);
    int rc = open_call(ctxs, n, stream);
    if (rc != CVH_OK) return rc;
    if (first) HIPCHK(lead, hipEventRecord(first, lead->stream));
    HIPCHK(lead, hipMemcpyAsync(db, hb, dev_bytes, hipMemcpyHostToDevice, lead->stream));
    rc = launches();
    if (rc != CVH_OK) return rc;
    rc = close_call(ctxs, n, stream, to_caller);
    if (rc != CVH_OK) return rc;
    if (wait) HIPCHK(lead, hipStreamSynchronize(lead->stream));
    return CVH_OK;
  }
};

// The plane sums of a call whose launch has written the planes of members 0 .. n-1, as cvh_set_image takes them: 8 integers per member in
// the call's device extra (zeroed with it; the kernel adds {sum p, sum p^2} per plane), and for the members whose stop norm the host
// takes (three channels) the planes themselves, fetched into the call's host-only part.  write_planes' own: plan() before
// MemberCall::begin(.., sums_bytes, fetch_bytes); fetch() inside run()'s launches, behind the kernel; arrive() behind the call's wait.
struct PlaneSums {
  cvh_context *const *ctxs = nullptr;
  int n = 0;
  size_t sums_bytes = 0, fetch_bytes = 0;
  std::vector<int> on_host;
  std::vector<size_t> fetch_off;

  void plan(cvh_context *const *ctxs_, int n_);
  unsigned long long *device_sums(const MemberCall &call, int i) const { return (unsigned long long *)(call.db + call.extra_off) + (size_t)8 * i; }
  int fetch(const MemberCall &call);
  void arrive(const MemberCall &call);
};
// the one path of a call that replaces the planes of ctxs[0 .. n_written-1] (an ingest, a conversion, a luma, local statistics, rank planes, smoothing, a restrict): see io_run.hip
int write_planes(cvh_context *const *ctxs, int n_written, int n_members, const char *what, void *stream,
                 const std::function<void(int, CvhIoMember &)> &fill, const std::function<int(const MemberCall &)> &launch,
                 size_t payload_bytes = 0, const std::function<void(int, void *)> &payload = nullptr);

// cvh_get_mask / cvh_get_mask_clean: into_d_mask() writes c->d_mask (allocated on first use) on c's stream; the bytes come down, one wait
template <class F>
int mask_to_host(cvh_context *c, uint8_t *mask, F into_d_mask)
{
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->d_mask) HIPCHK(c, hipMalloc((void **)&c->d_mask, c->n));
  const int rc = into_d_mask();
  if (rc != CVH_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(mask, c->d_mask, c->n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CVH_OK;
}

// nothing is thrown across the C boundary: a failed host allocation inside body() becomes CVH_ERR_NOMEM
template <class F>
int guarded(cvh_context *const *ctxs, int n, const char *what, F body)
{
  try { return body(); }
  catch (...) { return batch_fail(ctxs, n, CVH_ERR_NOMEM, "%s: out of host memory", what); }
}

// a single-context entry point that is a batch of one member: a NULL context is CVH_ERR_ARG without a message; body(what) is guarded
template <class F>
int guarded_one(cvh_context *c, const char *what, F body)
{
  return c ? guarded(&c, 1, what, [&]() { return body(what); }) : CVH_ERR_ARG;
}

// What launches(), which returns CVH_OK or an error already recorded with fail(), enqueues on c's stream, captured and instantiated into
// *out.  A capture that does not end in a graph fails with end_fmt (one %s: the HIP error).
template <class F>
int capture_graph(cvh_context *c, hipGraphExec_t *out, F launches, const char *end_fmt)
{
  HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  const int rc = launches();
  hipGraph_t graph = nullptr;
  const hipError_t e_end = hipStreamEndCapture(c->stream, &graph);
  if (rc != CVH_OK || e_end != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc != CVH_OK ? rc : fail(c, CVH_ERR_HIP, end_fmt, hipGetErrorString(e_end));
  }
  const hipError_t e_inst = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e_inst != hipSuccess) { *out = nullptr; return fail(c, CVH_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e_inst)); }
  return CVH_OK;
}
#pragma GCC visibility pop
