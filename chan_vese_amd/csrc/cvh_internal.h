// cvh_internal.h — shared declarations of the HIP implementation behind include/chanvese_hip.h.
// gfx950 (CDNA4, wave64) only.  Citations are file:line in the reference repository.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "chanvese_hip.h"

#define CVH_BLOCK 256  // 4 waves of 64

// Ablation / diagnostic keys of cvh_set_option (not part of include/chanvese_hip.h; defaults are what ships):
//   "wave_occupancy" waves per SIMD the 1-pixel wave kernel's grid is sized for (3..5; default 5; the 2-pixel kernel is built for 3),
//   "wave_depth" rows per group (4, 8), "wave_prio" s_setprio progress equalisation (0 off, 1 quarters,
//   2-4 thresholds crowded to the end, 5 clock-paced), "wave_sync" workgroup barrier per group (1),
//   "wave_imgv" 16-byte image pieces (1), "wave_xcd" XCD-contiguous workgroup numbering (1),
//   "wave_skew" per-mille strip-length skew of the 1-pixel kernel (0), "wave_cls" class-major workgroup numbering (0 off,
//   1 = 2-pixel kernel (default), 2 = 1-pixel kernel too), "wave_cskew" per-mille strip-length skew between dispatch rounds (500),
//   "wave_seam" 2-pixel kernel: a strip's final group without prefetch and park (1; 0 = with both: the same bits),
//   "wave_pol" = 2 (diagnostic value of the public option: plain stores with non-temporal loads),
//   "chain" fixed-point chained sums + deferred bookkeeping in the wave kernels (1), "far_terms" terms of the far-field series (5; 4), "wave_lds_cap", "wave_rev", "debug_times" (per-wave stamps
//   read with cvh_debug_read, tools/wave_timeline.py), "res_straight" (1; 0 = csv_resident_kernel's generic march whatever the tile height).

// Device-resident scalar state of one context.  Written only by the finalising workgroup
// of a kernel and read by the next kernel on the same stream (kernel boundary = visibility).
struct CvhState {
  double c1[CVH_MAX_CHANNELS];  // region means of the current u, used by the next step (:973)
  double c2[CVH_MAX_CHANNELS];  // (:974)
  double norm;                  // ||u_diff||_2 of the last executed step (:993)
  double stop_cond;             // (unused: the stop condition is a launch argument, CvhStepArgs::stop_cond)
  int steps_done;               // iterations executed since cvh_reset_run
  int stopped;                  // sticky: stop rule fired (:1000); later launches are no-ops
  unsigned ticket;              // arrival counter of the in-kernel finalisation
  int pending;                  // chain mode: the iteration of the last launch still awaits its bookkeeping (norm, stop test)
};

// Chain mode of the 2-pixel wave kernel (csv_wave2_kernel.hip): the two sums the NEXT iteration needs, sum (H - 1/2)
// and sum I (H - 1/2), are accumulated as 64-bit FIXED-POINT integers with agent-scope atomic adds -- integer addition
// is associative, so the result is bitwise reproducible whatever the arrival order -- into one of four rotating sets
// of 16 or 32 shards per sum (same-address atomics serialise at ~10 ns each; 765 workgroups over 32 shards do not queue).  Launch e
// reads set (e mod 4), adds into set (e+1 mod 4) and clears set (e+2 mod 4); nothing waits for a last workgroup.
// A set holds 64 integers: (1 + C) sums x 64 / (1 + C) shards (chain_device.h).
constexpr int CVH_CHAIN_SETS = 4;
struct CvhChainAcc { long long v[CVH_CHAIN_SETS][64]; };

// Resident kernel (csv_resident_kernel.hip): the words its workgroups synchronise on, zeroed before every launch.
constexpr int CVH_RESIDENT_MAX_TILES = 256;     // the master's eight waves watch 32 arrival lines each (one tile per CU: 256 on MI355X)
struct CvhResident {
  int error;            // a bounded wait gave up (a workgroup was not resident, or a fault): the launch drains, the host reports it
  unsigned pad[15];
  // three 16-byte pieces per tile {generation, 0, payload}, written with agent-scope stores: sum u_diff^2 of the tile (double), then its
  // fixed-point sums of H - 1/2 and I (H - 1/2) (chain_device.h's integers): the tile has finished iteration generation - 1 of the launch.
  // PIECE-MAJOR -- piece p of tile t at entry p * CVH_RESIDENT_MAX_TILES + t -- so that a poll instruction of the master reads 64 neighbouring
  // entries (1 KiB) and not 16 bytes of 64 different lines.  The master adds the integers itself (exact, order-free): no atomics inside the
  // launch, and the arrival does not wait for the border stores (arrivals on distinct addresses do not serialise)
  unsigned flag[CVH_RESIDENT_MAX_TILES * 16];
  // one 64-byte line per tile, written by the master as two 16-byte stores {generation, leave, c1} {generation, leave, c2}: the release
  // behind iteration generation - 1 and the region means of the level set it produced
  unsigned go[CVH_RESIDENT_MAX_TILES * 16];
  // one 64-byte line per tile {generation}: the tile's borders of iteration generation - 1 have reached memory (its neighbours wait for this)
  unsigned hflag[CVH_RESIDENT_MAX_TILES * 16];
  // ---- three channels only (csv_resident_kernel<3, .>), appended so that nothing the one-channel kernels address moves:
  // the FIFTH arrival piece of a tile {generation, 0, sum I_2 (H - 1/2)} (pieces 0 .. 3 -- sum u_diff^2, sum (H - 1/2), sum I_0 .., sum I_1 .. -- are `flag`'s four)
  unsigned flag_c3[CVH_RESIDENT_MAX_TILES * 4];
  // one 128-byte line per tile, six 16-byte pieces {generation, leave, c1_k} k = 0..2, {generation, leave, c2_k}: the three-channel release
  unsigned go_c3[CVH_RESIDENT_MAX_TILES * 32];
};
// what a one-channel launch and the Perona-Malik kernels (the error word only) need cleared
constexpr size_t CVH_RESIDENT_C1_BYTES = offsetof(CvhResident, flag_c3);

// Sums carried per workgroup and reduced in a fixed order (deterministic):
//   [0] sum H(u)  [1] sum (1-H(u))  [2..2+C) sum I_k H  [2+C..2+2C) sum I_k (1-H)  [2+2C] sum u_diff^2
__host__ __device__ constexpr int cvh_nsums(int C) { return 3 + 2 * C; }

// What a launcher WOULD launch (cvh_launch_info, include/chanvese_hip.h): filled at the launch site itself, by the
// same code path that selects the kernel flavour and the grid (CVH_LAUNCH below) -- nothing re-derives the choice.
struct CvhLaunchNote { char name[112]; unsigned grid, block, lds; };
void cvh_fill_note(CvhLaunchNote *note, unsigned grid, unsigned block, size_t lds, const char *fmt, ...);

struct CvhStepArgs {
  const double *u_in;
  double *u_out;
  const uint8_t *img[CVH_MAX_CHANNELS];
  unsigned img_stride;           // the planes are img[0] + k * img_stride (one slab)
  CvhState *st;
  double *partials;  // [nblocks][nsums]
  double *trace;     // [trace_cap][2C+1] or null
  int trace_cap;
  int h, w;
  int tiles_x, tiles_y;
  int nparts;        // number of partial rows the finaliser must add
  int fused_finalize;
  double alpha, beta, gamma;  // dt*mu, dt*(1/C), -nu*dt : addWeighted form of :985
  double eps;
  double lambda1[CVH_MAX_CHANNELS], lambda2[CVH_MAX_CHANNELS];
  // FAST flavour only
  const double *atan_tab;        // [2][CVH_ATAN_N]: atan(i/(N-1)) and pi/2 - atan(i/(N-1))
  double inv_eps;                // 1/eps
  double dk1, dk2;               // pi/eps, pi*eps : delta_eps(u) = 1 / (dk1*u^2 + dk2)
  double npix;                   // h*w
  double sum_img[CVH_MAX_CHANNELS];  // exact integer sums of the planes (complements are derived)
  double stop_cond;              // tol * ||mean_k I_k||_2 (:959), the value also held in CvhState
  double far_k[5], far_thr;      // wave kernels, FAST: far-field series of atan(eps/u)/pi (5 terms) and its threshold (32 eps)
  int derive_complement;         // sums [1] and [2+C..] are N - sum H, sum I - sum I H; 2: sums [0], [2..] are of H - 1/2
  int tile_rows;                 // rows per tile of the step kernel
  int use_lut;
  int use_dma;                   // LDS-DMA tile loader (even widths)
  int strip_rows;                // rows per workgroup (strip kernel) / per wave (wave kernel)
  const double *atan2_tab;       // [CVH_ATAN2_N]: (pi/4 + atan((j-128)/128)) / pi
  int wave_minw;                 // waves per SIMD the wave kernel is compiled for (5..8)
  unsigned long long *dbg_times; // diagnostic: per-wave {start, end, hw id} stamps (100 MHz), or null
  int *host_status;              // pinned host memory {steps_done, stopped}: written by the finaliser, polled by the host
  double *dummy;                 // >= max(w, 64) doubles that nobody reads: target of masked-off lanes' stores
  int wave_imgv;                 // wave kernel: 16-byte image pieces through LDS (w % 16 == 0)
  int wave_xcd;                  // wave kernel: XCD-contiguous workgroup numbering
  int wave_rev;                  // diagnostic: oldest workgroups take the bottom strips
  const int *strip_bounds;       // wave kernel: first row of each strip, [tiles_y + 1]
  int wave_depth;                // wave kernel: rows of u kept in flight per lane (4 or 8)
  int wave_sync;                 // wave kernel: workgroup barrier every 4 rows
  int wave_prio;                 // progress-based s_setprio in the wave kernel
  int state32;                   // 2-pixel wave kernel: the level set lives in HBM as float (option "state" = 32; u_in / u_out then point at floats)
  int near_switch;               // FAST wave / resident kernels: a wave that met near-field pixels runs its next group of rows in the table form of H_eps
  int wave_lds_cap;              // pad the LDS request so that at most wave_minw workgroups fit a CU
  CvhChainAcc *chain;            // chain mode (2-pixel wave kernel, FAST): fixed-point sum sets, or null
  int chain_phase;               // set this launch reads
  int chain_pb;                  // set that held the sums of u when the run counter was last reset (flush: set = pb + steps_done)
  double chain_scale[4], chain_inv[4];   // powers of two: fixed-point scale of sum (H-1/2), sum I_k (H-1/2) and their inverses
  double *chain_s4;              // [2][nparts] per-workgroup sum u_diff^2 rows, by launch parity
  int wave_pol;                  // 2-pixel wave kernel: cache policy of the level-set rows (wave2_device.h): 1 write-through stores, 0 plain
  int wave_cls;                  // 2-pixel wave kernel: workgroups per XCD per dispatch round (= CUs per XCD); > 0 numbers the
                                 // workgroups class-major (round 0 of every XCD first), 0 = plain XCD-contiguous numbering
  int wave_seam;                 // 2-pixel wave kernel, FAST: a strip's final group neither prefetches nor parks (csv_wave2_body.inc); 0 = it does,
                                 // as every other group
  CvhLaunchNote *note;           // host only: non-null = describe the launch instead of issuing it (CVH_LAUNCH)
  // resident kernel (csv_resident_kernel.hip): tiles_x x tiles_y tiles, one workgroup each
  CvhResident *resident;         // synchronisation words
  double *res_halo;              // [2][tiles][6 * 128] border rows / columns of every tile, by iteration parity
  int res_steps, res_poll_cap;   // iterations in this launch; polls before a wait gives up
  int res_t0;                    // index of the launch's first iteration inside the run (= iterations enqueued before it)
  int res_prio;                  // resident kernels: a wave lowers its priority with every quarter of its band (the two waves of a SIMD finish together)
  int res_band_rows;             // rows per wave when every tile has 8 x that many rows (2, 4, 8, 16: straight-line march), else 0
  int res_go_shift;              // 2^shift tiles of one XCD share a release line (csv_resident_kernel.hip, go_line)
  // one-buffer flow of the 2-pixel wave kernel (csv_wave2_ob_kernel, csv_wave2_kernel.hip; cvh_ob_* below): u_in == u_out == the padded slab
  int one_buffer;                // 1: this launch updates the level set in place
  int ob_pitch;                  // doubles per row of the slab: w columns + the column shadow (cvh_ob_pitch)
  int ob_rows;                   // rows of the slab: h of the plane + 2 x 3 shadow rows per strip
  int ob_par;                    // parity of the shadow this launch READS (it writes the other one)
  const int *ob_tab;             // [tiles_y][CVH_OB_TAB] shadow-row table of the strips (cvh_ob_fill_table)
};

// One-buffer flow: the slab's layout, shared by the kernel, the pack / unpack kernels and the host.
//   row r of the plane (pitch doubles): [w columns][parity 0: per wave-column {A.x A.y B.x B.y}][parity 1: the same] -- A is the pair of
//   the wave-column's lane 63 (the halo pair of its east neighbour's lane 0), B the pair of its lane 1 (B.x is the east extra of its west
//   neighbour); behind the h rows, per parity and strip three shadow rows: rows s0 - 2, s0 - 1 and s1 of the strip as they were when the
//   iteration of that parity began.  Parity p of the pads and shadow rows belongs to the iterations that read buffer p of the pair.
#define CVH_OB_TAB 8   // ints per strip: [0] where its first row goes, [1] [2] [4] where its last row goes, [3] its last row but one (shadow-row
                       // index strip * 3 + j, -1 none); [5 .. 7] the plane rows its own three shadow rows are copies of (-1 none)
__host__ __device__ constexpr int cvh_ob_pitch(int w, int nwc) { return (w + 8 * nwc + 15) & ~15; }
__host__ __device__ constexpr int cvh_ob_slot(int w, int nwc, int par, int wc, int b) { return w + 4 * nwc * par + 4 * wc + 2 * b; }   // in doubles
__host__ __device__ constexpr int cvh_ob_rows(int h, int nstrips) { return h + 6 * nstrips; }
__host__ __device__ constexpr int cvh_ob_shadow_row(int h, int nstrips, int par, int idx) { return h + 3 * nstrips * par + idx; }

// Fused batch (cvh_enqueue_steps_batch, api.hip): one grid holds the sections of several contexts, each the context's own grid
// (nparts workgroups + the chain-mode bookkeeper) padded to a multiple of 8 workgroups, so that blockIdx.x & 7 still names the
// XCD the member-local numbering assumes.  map[blockIdx.x / 8] names the member and where its section starts; args[member] is
// that member's launch arguments (read through the scalar cache).  Workgroups past a section's nblk are padding and exit.
struct CvhBatchEntry { unsigned member, first, nblk, pad; };
struct CvhBatchArgs { const CvhBatchEntry *map; const CvhStepArgs *args; };
struct CvhBatchLaunch { CvhBatchArgs k; unsigned grid; };   // host: what the batch entry point of a launcher is given

// The ONE way a step / Perona-Malik kernel is launched: KERNEL may be a parenthesised template-id; the trailing
// arguments are a printf format + values that spell the instantiation as rocprofv3 prints it.
#define CVH_LAUNCH(KERNEL, GRID, LDS, S, A, ...)                                                  \
  do {                                                                                             \
    if ((A).note) cvh_fill_note((A).note, (unsigned)(GRID), CVH_BLOCK, (size_t)(LDS), __VA_ARGS__); \
    else hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(CVH_BLOCK), (LDS), (S), (A));                 \
  } while (0)
// The same, for a kernel that also has a batch entry point BKERNEL: B non-null launches that over B's grid instead
#define CVH_LAUNCH_B(KERNEL, BKERNEL, GRID, LDS, S, A, B, ...)                                   \
  do {                                                                                             \
    if ((A).note) cvh_fill_note((A).note, (unsigned)(GRID), CVH_BLOCK, (size_t)(LDS), __VA_ARGS__); \
    else if (B) hipLaunchKernelGGL(BKERNEL, dim3((B)->grid), dim3(CVH_BLOCK), (LDS), (S), (B)->k);   \
    else hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(CVH_BLOCK), (LDS), (S), (A));                 \
  } while (0)
#define CVH_TF(b) ((b) ? "true" : "false")

#define CVH_ATAN_N 129
#define CVH_ATAN2_N 257

struct CvhPmArgs {
  const double *in;
  double *out;
  int h, w;
  int tiles_x, tiles_y;
  double K2;  // K*K (:520)
  double L;
  double invK2, L4;  // FAST flavour: 1/K^2, L/4
  int fast;
  int strip_rows;    // wave kernel: rows per wave
  int pol;           // 2-step wave kernel: 1 = write-through stores (the state planes fit the Infinity Cache), 0 = plain
  // resident kernel (pm_resident_kernel.hip): tiles_y x tiles_x tiles, one workgroup each, res_steps time steps in one launch
  CvhResident *resident;         // the error word
  double *res_halo;              // 2 x tiles x 1024 entries of 16 bytes {value, tag}: the tiles' borders, double-buffered by step parity
  unsigned res_serial;           // tag of this launch (entries left by earlier launches never match)
  int res_steps;
  int res_band_rows;             // rows per wave: 2, 4, 8 or 16 (tiles of 8 x that many rows)
  int res_prio;                  // a wave lowers its priority with every quarter of its band (csv_resident_kernel.hip, quarter_prio)
  int res_poll_cap;              // polls before a wait gives up
  unsigned long long *dbg_times; // diagnostic (option "debug_times", tools/pm_resident_timeline.py): 12 stamps per workgroup, or null
  CvhLaunchNote *note;   // host only: describe the launch instead of issuing it (CVH_LAUNCH)
};

// Perona-Malik batch (cvh_perona_malik_batch, api.hip): the planes of several contexts in ONE cooperative launch of pm_resident_batch_kernel.
// Plane p owns the tiles_y x tiles_x workgroups tile_base .. tile_base + tiles - 1 of the grid (row-major inside the plane); map[wg] = p.
// The border buffer holds the launch's ntiles tiles per step parity, a plane's tiles at the plane's tile_base.  Uploaded by the host.
struct CvhPmBatchPlane { CvhPmArgs a; int tile_base, pad; };
struct CvhPmBatchArgs { const CvhPmBatchPlane *planes; const unsigned *map; int ntiles, nplanes; };
// uint8 plane <-> FP64 state of one plane of a batch's load / store launch
struct CvhPmIoPlane { uint8_t *img; double *state; unsigned long long n; };

// Device-memory I/O (io_kernels.hip, io_run.hip) and reinitialisation (reinit_kernels.hip): one entry per member of a batch kernel's grid.
// A kernel reads the fields its operation names; the host leaves the others zero.  The table lives in the leader's device table, 16-byte
// aligned entries.
struct CvhIoMember {
  const void *src;                    // ingest: the caller's bytes; mask, reinit: the level set (double); checkerboard: the h row factors
  const void *src2;                   // checkerboard: the w column factors; smoothing: the pair's taps
  void *dst;                          // mask / interleaved planes out: the caller's buffer; checkerboard, reinit: the level set written
  uint8_t *plane[CVH_MAX_CHANNELS];   // the context's planes (ingest: written; planes out: read); reinit: [0] the class words of the
                                      // bands, [1] the distance fields (the context's workspace)
  unsigned long long *sums;           // ingest: {sum p, sum p^2} per plane, zeroed before the launch; reinit: the flag word, zeroed
                                      // (bit 0: an outside pixel exists, bit 1: an inside pixel exists)
  int *state_zero;                    // checkerboard, reinit: the four run words of CvhState a new run clears (steps_done, stopped, ticket, pending)
  long long *chain_zero;              // checkerboard, reinit: the chain-mode sum set a new run clears (64 integers)
  unsigned long long n;               // pixels
  int h, w, C;
  int interleaved;                    // ingest: the source is h * w * C interleaved bytes (planar otherwise)
  unsigned first, nblk;               // workgroups first .. first + nblk - 1 of the grid are this member's (first ascending, member 0 at 0)
  int h2, w2;                         // restrict: the fine grid the member's planes (h x w) are averaged from, src its first plane
  unsigned long long src_stride;      // restrict, luma: bytes between the planes of the source context
};

// ---- launchers (csv_kernels.hip / pm_kernels.hip / misc_kernels.hip / io_kernels.hip) ----
unsigned cvh_io_blocks(size_t n);                    // workgroups of a member in the ingest / mask / planes-out grids
unsigned cvh_io_checkerboard_blocks(int h, int w);
hipError_t cvh_launch_io_ingest(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_image_sums(const uint8_t *const *planes, int channels, size_t n, unsigned long long *out /* [2 * channels], zeroed */,
                                 hipStream_t s);   // the ingest's sums of planes already on the device
hipError_t cvh_launch_io_checkerboard(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_io_mask(const CvhIoMember *tab, int nmem, unsigned grid, int invert, hipStream_t s);
hipError_t cvh_launch_io_image_out3(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_io_narrow(const double *u, float *out, size_t n, hipStream_t s);   // out = (float)u
// reinitialisation (reinit_kernels.hip): bands of CVH_REINIT_BAND rows in the column pass (one class word per band and column), rows of up to
// CVH_REINIT_LDS_COLS columns staged in LDS by the row pass (8 bytes per column: 64 KiB)
#define CVH_REINIT_BAND 32
#define CVH_REINIT_LDS_COLS 8192
unsigned cvh_reinit_column_blocks(int h, int w);     // workgroups of a member in the two column launches
unsigned cvh_reinit_row_blocks(int h);               // and in the row launch
size_t cvh_reinit_bits_bytes(int h, int w);          // the class words' share of the workspace (the distance fields follow)
size_t cvh_reinit_workspace_bytes(int h, int w);
hipError_t cvh_launch_reinit(const CvhIoMember *cols, unsigned col_grid, const CvhIoMember *rows, unsigned row_grid, int nmem, int max_w,
                             hipStream_t s);
// connected components (components_kernels.hip): a member's section is one lane per pixel; plane[0] the parent words, plane[1] the per-root
// statistics, plane[2] one count per workgroup (the context's workspace); sums: the member's word (K; keep_largest's bid), zeroed; dst the
// label plane (may be null), the mask bytes, or the rows of the table
unsigned cvh_cc_blocks(size_t n);
size_t cvh_cc_workspace_bytes(size_t n);
hipError_t cvh_launch_cc_label(const CvhIoMember *tab, int nmem, unsigned grid, int conn, int invert, bool any_labels, hipStream_t s);
hipError_t cvh_launch_cc_table(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_cc_clean(const CvhIoMember *tab, int nmem, unsigned grid, int conn, int invert, unsigned min_area, long fill_holes,
                               int keep_largest, hipStream_t s);
hipError_t cvh_launch_cc_number(const CvhIoMember *tab, int nmem, unsigned grid, int mode, int conn, int invert, hipStream_t s);
// component measures (measure_kernels.hip), behind cvh_launch_cc_number.  The numbering launches read the member table above (plane[] the
// workspace); the measure launches read a SECOND table of the same members, because they need the image as well: src the parent words of
// the numbered forest (the workspace's first plane), plane[] the context's C image planes, dst the member's rows (cvh_region), h2 the
// number of rows dst holds -- min(K, cap); 0: the member's workgroups return at once --, sections of cvh_measure_blocks(n) workgroups,
// CVH_MEASURE_TILE pixels in flat raster order each.  any_c1 / any_c3: a member with one / three channels exists (one launch each).
#define CVH_MEASURE_TILE 8192
unsigned cvh_measure_blocks(size_t n);
hipError_t cvh_launch_measure(const CvhIoMember *tab, int nmem, unsigned grid, bool any_c1, bool any_c3, hipStream_t s);
// component overlaps (overlap_kernels.hip), behind cvh_launch_cc_number, on a SECOND table of the same members in sections of
// cvh_measure_blocks(n) workgroups: src the parent words of the numbered forest, src2 the caller's int32 plane, dst the member's
// src_stride slots (a power of two; cleared by the host), plane[0] the src_stride / 2 rows behind them (cvh_overlap, unsorted), sums the
// member's CVH_OVERLAP_CTL 32-bit control words, zeroed: slots claimed (P), overflow, rows written; w2 != 0: rows are asked for;
// h2 != 0: the member sits the launch out (a second launch for the members whose table overflowed).  An empty slot has key 0; the key of
// (a, b) is ((a + 1) << 32) | (uint32_t)b.
struct CvhOverlapSlot { unsigned long long key; unsigned count, pad; };
#define CVH_OVERLAP_CTL 4
hipError_t cvh_launch_overlap(const CvhIoMember *tab, int nmem, unsigned grid, bool any_rows, hipStream_t s);
// contours (contour_kernels.hip, whose head comment describes a member's entry).  The pixel launches take sections of cvh_cc_blocks(n)
// workgroups; behind the host's wait for E the edge launches take sections of cvh_contour_edge_blocks(E, n) workgroups (none for a member
// without edges), a lane per edge -- or per pixel -- and trip.  The per-pixel workspace is [mask bytes][edge sets][prefix words][a count
// per 256 pixels] at the offsets below; the per-edge workspace, sized for `cap` edges, holds the loops' rows at cvh_contour_rows_offset.
unsigned cvh_contour_scan_trip();                    // counts the one-wave scan of a member takes per trip
unsigned cvh_contour_edge_blocks(size_t edges, size_t n);
size_t cvh_contour_bits_offset(size_t n);
size_t cvh_contour_prefix_offset(size_t n);
size_t cvh_contour_counts_offset(size_t n);
size_t cvh_contour_pixel_bytes(size_t n);
size_t cvh_contour_edge_bytes(size_t cap);
size_t cvh_contour_rows_offset(size_t cap);
hipError_t cvh_launch_contours_count(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_contours_trace(const CvhIoMember *tab, int nmem, unsigned grid, int conn, int simplify, int rounds, bool any_points,
                                     const CvhIoMember *levels /* null: lattice points; else subpixel points from these level sets */, int invert,
                                     hipStream_t s);
// device-side initial level sets (init_kernels.hip).  Histogram: plane[] the member's planes, sums its 255 C + 1 32-bit counters (zeroed
// by the host), sections of cvh_io_blocks(n) workgroups.  Start: dst the level set written, plane[] read by the threshold mode,
// state_zero / chain_zero as the checkerboard's; member i's start is par[i], a table behind the member table:
//   CVH_START_THRESHOLD  inside where g > a
//   CVH_START_RECT       inside where a <= col < b and c <= row < d (the host has clipped the rectangle to the plane)
//   CVH_START_DISK       inside where (col - a)^2 + (row - b)^2 <= c^2, 0 <= c < 2^31
#define CVH_HIST_MAX_BINS (255 * CVH_MAX_CHANNELS + 1)
enum { CVH_START_THRESHOLD = 0, CVH_START_RECT = 1, CVH_START_DISK = 2 };
struct CvhInitStart { double inside, outside; long long a, b, c, d; int mode, pad; };
unsigned cvh_init_start_blocks(size_t n);
hipError_t cvh_launch_init_histogram(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_init_start(const CvhIoMember *tab, const CvhInitStart *par, int nmem, unsigned grid, hipStream_t s);
// coarse-to-fine (pyramid_kernels.hip).  Restrict: plane[] the coarse member's planes (written), src / src_stride / h2 / w2 the fine
// planes, sums as the ingest's.  Prolong: src the coarse level set ((h + 1) / 2 x (w + 1) / 2 doubles), dst the fine one (h x w),
// state_zero / chain_zero as the checkerboard's.
size_t cvh_restrict_items(int fine_h, int fine_w);   // what a pair's lanes share out, an item per lane and trip
size_t cvh_prolong_items(int fine_h, int fine_w);
unsigned cvh_restrict_blocks(int fine_h, int fine_w);
unsigned cvh_prolong_blocks(int fine_h, int fine_w);
hipError_t cvh_launch_restrict(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_prolong(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
// colour spaces (colour_kernels.hip).  Convert: plane[] the member's three planes, replaced in place, sums as the ingest's.  Luma:
// src / src_stride the three planes of the source, plane[0] the member's single plane (written), sums as the ingest's.  space, order
// and inverse are the call's (include/chanvese_hip.h).  A lane takes a 16-byte piece per trip, CVH_COLOUR_BLOCK_PIXELS a workgroup.
#define CVH_COLOUR_BLOCK_PIXELS (16 * CVH_BLOCK)
unsigned cvh_colour_blocks(size_t n);
hipError_t cvh_launch_colour_convert(const CvhIoMember *tab, int nmem, unsigned grid, int space, int order, int inverse, hipStream_t s);
hipError_t cvh_launch_colour_luma(const CvhIoMember *tab, int nmem, unsigned grid, int order, hipStream_t s);
// windowed planes (window_device.h; local_kernels.hip, rank_kernels.hip).  src / src_stride the planes of the source context and w2
// their number; plane[] the member's C planes (written), sums as the ingest's; h2 the radius; interleaved the member's codes, a family's
// bits per code apart; dst the member's workspace, rows cvh_window_pitch(w) entries apart.  A family's launches read ONE table: in a
// row pass a workgroup takes a row segment of CVH_WINDOW_SEGMENT columns per trip, in a column pass a wave takes a band of rows
// (CVH_WINDOW_BAND, or a family's own) x CVH_WINDOW_STRIP columns per trip.
#define CVH_WINDOW_SEGMENT 1024
#define CVH_WINDOW_BAND 32
#define CVH_WINDOW_STRIP 256
// (the geometry's earlier names, used by no code: tests/test_rank_api.py pins the two CVH_RANK_ lines -- the rank passes take the local ones' geometry)
#define CVH_LOCAL_SEGMENT CVH_WINDOW_SEGMENT
#define CVH_LOCAL_BAND CVH_WINDOW_BAND
#define CVH_RANK_SEGMENT CVH_LOCAL_SEGMENT
#define CVH_RANK_BAND CVH_LOCAL_BAND
__host__ __device__ constexpr size_t cvh_window_pitch(int w) { return ((size_t)w + 3) & ~(size_t)3; }   // whole words per lane of a column pass
// local statistics (local_kernels.hip): codes what[k] << 2 k; the workspace a slot of cvh_local_slot_bytes(h, w) per source plane, the
// row sums of p^2 (32-bit) and behind them those of p (16-bit).  Two launches: the row pass where a pair has `passes`, and the column pass.
__host__ __device__ constexpr size_t cvh_local_slot_bytes(int h, int w) { return (6 * (size_t)h * cvh_window_pitch(w) + 15) & ~(size_t)15; }
unsigned cvh_local_blocks(int h, int w, int planes_read);
hipError_t cvh_launch_local(const CvhIoMember *tab, int nmem, unsigned grid, unsigned passes, hipStream_t s);
// rank planes (rank_kernels.hip): codes what[k] << 3 k; the workspace CVH_RANK_SLOTS byte planes of cvh_rank_slot_bytes(h, w) per source
// plane (rank_kernels.hip says which is which).  Up to five launches, chosen by `passes`: the row pass of every chain
// (CVH_RANK_PASS_ROWS), the column and the second row pass of the chains that run twice (CVH_RANK_PASS_TWICE), the median
// (CVH_RANK_PASS_MEDIAN), and always the final pass, which writes the planes.  The column passes' band is
// cvh_rank_band_rows(R, CVH_WINDOW_BAND) rows (rank_math.h); the median takes CVH_RANK_MEDIAN_BAND rows x CVH_RANK_MEDIAN_STRIP columns
// per wave and trip.
#define CVH_RANK_MEDIAN_BAND 32
#define CVH_RANK_MEDIAN_STRIP 64
#define CVH_RANK_SLOTS 7
#define CVH_RANK_PASS_ROWS 1u
#define CVH_RANK_PASS_TWICE 2u
#define CVH_RANK_PASS_MEDIAN 4u
__host__ __device__ constexpr size_t cvh_rank_slot_bytes(int h, int w) { return ((size_t)h * cvh_window_pitch(w) + 255) & ~(size_t)255; }
unsigned cvh_rank_blocks(int h, int w, int R, int row_jobs, int median_planes);
hipError_t cvh_launch_rank(const CvhIoMember *tab, int nmem, unsigned grid, unsigned passes, hipStream_t s);
// smoothing (smooth_kernels.hip): codes what[k] << 2 k; src2 the pair's payload, CVH_SMOOTH_TAPS taps of 16 bits (zero behind the radius);
// the workspace a slot of cvh_smooth_slot_bytes(h, w) per source plane, the row pass's 8.8 fixed-point values.  Two launches: the row
// pass where a pair has `passes`, and the column pass, in which a WORKGROUP takes a band of cvh_smooth_band_rows(R) rows x
// CVH_SMOOTH_STRIP columns per trip: the band and R rows on either side are the CVH_SMOOTH_TILE_ROWS rows of its LDS tile.
#define CVH_SMOOTH_TAPS (CVH_SMOOTH_RADIUS_MAX + 1)
#define CVH_SMOOTH_STRIP 64
#define CVH_SMOOTH_TILE_ROWS 256
__host__ __device__ constexpr int cvh_smooth_band_rows(int R) { return CVH_SMOOTH_TILE_ROWS - 2 * R; }
__host__ __device__ constexpr size_t cvh_smooth_slot_bytes(int h, int w) { return (2 * (size_t)h * cvh_window_pitch(w) + 15) & ~(size_t)15; }
unsigned cvh_smooth_blocks(int h, int w, int R, int planes_read);
hipError_t cvh_launch_smooth(const CvhIoMember *tab, int nmem, unsigned grid, unsigned passes, hipStream_t s);
// energy (energy_kernels.hip).  src the level set, src2 the CvhState that holds its means, plane[] the planes, dst the member's item rows
// (cvh_energy_items x CVH_ENERGY_SLOTS doubles of the context's workspace), sums a row of CVH_ENERGY_ROW doubles: [0] eps (read), then
// length, area, fit_in[3], fit_out[3], c1[3], c2[3] (written).  An item is CVH_ENERGY_BAND rows x CVH_ENERGY_COLS columns, a wave's trip.
#define CVH_ENERGY_BAND 32
#define CVH_ENERGY_COLS 128
#define CVH_ENERGY_SLOTS (2 + 2 * CVH_MAX_CHANNELS)
#define CVH_ENERGY_ROW 16
__host__ __device__ constexpr unsigned cvh_energy_items(int h, int w)
{
  return (((unsigned)h + CVH_ENERGY_BAND - 1) / CVH_ENERGY_BAND) * (((unsigned)w + CVH_ENERGY_COLS - 1) / CVH_ENERGY_COLS);
}
unsigned cvh_energy_blocks(int h, int w);
hipError_t cvh_launch_energy(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);   // the term pass, then the reduce pass
// mask scores (score_kernels.hip).  src the level set, src2 the truth bytes, plane[0] the member's four planes of band words (class of the
// mask, class of the truth, surface of the mask, surface of the truth: cvh_score_words_bytes apart), plane[1] the two vertical distance
// fields (one unsigned per pixel: low half to the nearest pixel of surf(T) in the column, high half to surf(M), 0xffff = none) -- the
// context's workspace --, sums the member's result row of CVH_SCORE_ROW 64-bit words, zeroed: tp, fp, fn, tn, surf_m, surf_t, within_m,
// within_t, dist_m_q16, dist_t_q16, hd2_m, hd2_t (the maxima in the words' low halves).  Bands and chunks are the reinitialisation's.
#define CVH_SCORE_ROW 16
enum { CVH_SCORE_TP, CVH_SCORE_FP, CVH_SCORE_FN, CVH_SCORE_TN, CVH_SCORE_SURF_M, CVH_SCORE_SURF_T, CVH_SCORE_WITHIN_M, CVH_SCORE_WITHIN_T,
       CVH_SCORE_DIST_M, CVH_SCORE_DIST_T, CVH_SCORE_HD2_M, CVH_SCORE_HD2_T };
__host__ __device__ constexpr size_t cvh_score_words_bytes(int h, int w)
{
  return ((size_t)((h + CVH_REINIT_BAND - 1) / CVH_REINIT_BAND) * (size_t)w * sizeof(unsigned) + 255) & ~(size_t)255;
}
// bytes of a member's workspace: [four planes of band words][distance fields][truth plane of the host form]
inline size_t cvh_score_truth_offset(int h, int w) { return 4 * cvh_score_words_bytes(h, w) + (size_t)h * (size_t)w * sizeof(unsigned); }
inline size_t cvh_score_workspace_bytes(int h, int w) { return cvh_score_truth_offset(h, w) + (size_t)h * (size_t)w; }
// the four launches of one call: cols / rows are the member tables of launches 1 - 3 and of launch 4 (cvh_reinit_column_blocks /
// cvh_reinit_row_blocks workgroups per member), max_w the widest member (sizes the LDS window of launch 4)
hipError_t cvh_launch_score(const CvhIoMember *cols, unsigned col_grid, const CvhIoMember *rows, unsigned row_grid, int nmem, int max_w,
                            int invert, unsigned tol2, hipStream_t s);
// mask morphology and mask starts (morph_kernels.hip).  Three tables of the same members.  The mask launches' (cvh_launch_io_mask /
// cvh_launch_cc_clean, only where the call cleans): dst the member's byte plane.  The column table (cvh_reinit_column_blocks workgroups per
// member): src the level set, src2 the byte plane of the cleaned mask, plane[0] / plane[1] the two planes of band words the passes ping-pong
// between (cvh_score_words_bytes each), plane[2] the vertical distance field (one 16-bit word per pixel, 0xffff = none within reach).  The
// emit table (cvh_io_blocks workgroups per member, 16 pixels per lane and trip): plane[0] the band words of the result, or src bytes at any
// alignment (nonzero = set: a mask start); dst bytes at any alignment, or the level set with state_zero / chain_zero as the checkerboard's.
// par[i] is member i's: the squared radius, its integer root, and the two doubles of a level-set write.
struct CvhMorphPar { double inside, outside; unsigned r2, root, pad[2]; };
// bytes of a member's workspace: [two planes of band words][distance field][byte plane: the cleaned mask, or the bytes a host form stages]
inline size_t cvh_morph_dist_offset(int h, int w) { return 2 * cvh_score_words_bytes(h, w); }
inline size_t cvh_morph_bytes_offset(int h, int w) { return cvh_morph_dist_offset(h, w) + (((size_t)h * (size_t)w * sizeof(unsigned short) + 255) & ~(size_t)255); }
inline size_t cvh_morph_workspace_bytes(int h, int w) { return cvh_morph_bytes_offset(h, w) + (size_t)h * (size_t)w; }
// the band words of the start set into plane[0]: from the level set (cvh_get_mask's rule, invert applied) or from the byte plane
hipError_t cvh_launch_morph_bits(const CvhIoMember *cols, int nmem, unsigned col_grid, bool from_levelset, int invert, hipStream_t s);
// pass k = 0 .. npass-1 reads plane[k & 1] and writes plane[(k + 1) & 1]: a dilation by D(r2), of the complement within the plane where
// complement[k] (an erosion).  Two launches per pass, ordered by kernel boundaries
hipError_t cvh_launch_morph_passes(const CvhIoMember *cols, const CvhMorphPar *par, int nmem, unsigned col_grid, int npass, const bool *complement,
                                   hipStream_t s);
hipError_t cvh_launch_morph_emit(const CvhIoMember *tab, const CvhMorphPar *par, int nmem, unsigned grid, bool from_bytes, bool to_levelset,
                                 hipStream_t s);
// object split (split_kernels.hip, whose head comment names every table's fields).  The growth's key plane is the member's plane rounded
// up to whole tiles of CVH_SPLIT_TILE_ROWS x CVH_SPLIT_TILE_COLS 64-bit keys (the context's workspace, the padding zero); the sweeps are
// enqueued CVH_SPLIT_GROUP at a time, sweep j reading the members' counters of slot j and adding to those of slot j + 1 (32-bit words,
// nmem apart).  The pixel launches take sections of cvh_cc_blocks(n) workgroups, the sweeps one workgroup per tile, the emit launch
// cvh_split_emit_blocks(n).
#define CVH_SPLIT_TILE_ROWS 32
#define CVH_SPLIT_TILE_COLS 64
#define CVH_SPLIT_GROUP 4
inline int cvh_split_tiles_y(int h) { return (h + CVH_SPLIT_TILE_ROWS - 1) / CVH_SPLIT_TILE_ROWS; }
inline int cvh_split_tiles_x(int w) { return (w + CVH_SPLIT_TILE_COLS - 1) / CVH_SPLIT_TILE_COLS; }
inline size_t cvh_split_workspace_bytes(int h, int w)
{
  return (size_t)cvh_split_tiles_y(h) * CVH_SPLIT_TILE_ROWS * (size_t)cvh_split_tiles_x(w) * CVH_SPLIT_TILE_COLS * sizeof(unsigned long long);
}
unsigned cvh_split_emit_blocks(size_t n);
hipError_t cvh_launch_split_markers(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_split_keys(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_split_sweeps(const CvhIoMember *tiles, int nmem, unsigned tile_grid, int conn, int sweeps, hipStream_t s);
hipError_t cvh_launch_split_emit(const CvhIoMember *tab, const CvhMorphPar *par, int nmem, unsigned grid, bool to_levelset, hipStream_t s);
hipError_t cvh_launch_split_table(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
// the marching wave of the four-phase and localised step kernels (march_device.h) and what their host flows share (march_run.hip)
#define CVH_MARCH_COLS 61       // output columns per wave: lanes 2 .. 62 (lanes 0, 1 and 63 hold the strip's halo columns)
#define CVH_MARCH_TARGET_WAVES 4096
#define CVH_MARCH_MIN_ROWS 8
// rows per item of a plane of h rows and nwc wave-columns: enough item rows for about CVH_MARCH_TARGET_WAVES waves, a multiple of four
// rows, at least CVH_MARCH_MIN_ROWS.  A function of the shape ALONE -- not of the device -- because the sums' order follows it.
inline int cvh_march_rows(int h, int nwc)
{
  const int target = CVH_MARCH_TARGET_WAVES / nwc > 1 ? CVH_MARCH_TARGET_WAVES / nwc : 1;
  int rows = (int)(((long long)h + target - 1) / target);
  rows = (int)(((long long)rows + 3) & ~3ll);
  return rows > CVH_MARCH_MIN_ROWS ? rows : CVH_MARCH_MIN_ROWS;
}
// the head of both state blocks: what the host's chunk loop reads without knowing the model
struct CvhMarchCount {
  int steps_done;                  // iterations executed in this call
  int stopped;                     // sticky: the stop rule fired; every later launch of the call returns at once
};
// the FAST forms' constants, from eps / far_terms / the context's atan tables (fill_front_args)
struct CvhFrontArgs {
  double eps, inv_eps, dk1;        // FAST: 1 / eps, pi / eps
  double far_k[5], far_thr;        // FAST: far-field series of H_eps (wave_math.h)
  const double *atan2_tab;         // FAST: [CVH_ATAN2_N]
};
// four phases (multiphase_kernels.hip; include/chanvese_hip.h, "Four phases").  A wave's ITEM is a strip of strip_rows rows x
// CVH_MARCH_COLS columns of the plane; the partition -- hence every sum -- is a function of the shape alone (cvh_mp_geometry).  An item's
// row of partial sums holds cvh_mp_nsums(C) doubles:
//   [0..4) sum w11, w10, w01, w00   [4 + ab C + k] sum I_k w_ab (ab = 0..3 in that order)   [4 + 4C] sum d1^2   [5 + 4C] sum d2^2
// The pair's state block lives in A's workspace and is written by the one-workgroup finalise launch alone.
__host__ __device__ constexpr int cvh_mp_nsums(int C) { return 6 + 4 * C; }
struct CvhMpGeom { int nwc, strip_rows, nstrips, nitems; unsigned grid; };
CvhMpGeom cvh_mp_geometry(int h, int w);
struct CvhMpState {
  CvhMarchCount run;
  double c[4][CVH_MAX_CHANNELS];   // c11, c10, c01, c00: the means of the current pair, read by the next iteration
  double norm[2];                  // ||d1||_2, ||d2||_2 of the last executed iteration
};
// A member (pair) of a four-phase launch: the kernels read a device table of these records (constant address space: a wave-uniform
// record comes in scalar loads, as a by-value kernel argument does), a workgroup finds its record through `first`, the prefix block
// counts of the step grid.  A launch of parity p reads u[e][p] and writes u[e][p ^ 1]: the table is uploaded once per call.
struct CvhMpArgs {
  double *u[2][2];                 // [parity][phi1, phi2]: both buffers of both level sets (by value: u[0] read, u[1] written)
  const uint8_t *img[CVH_MAX_CHANNELS];
  CvhMpState *st;                  // the pair's own state block (A's workspace)
  double *partials;                // [nitems][cvh_mp_nsums(C)]
  double *trace;                   // [trace_cap][4C + 2] or null
  int trace_cap;
  int h, w;
  CvhMpGeom g;
  double alpha[2], beta[2], gamma[2];          // dt mu, dt / C, -dt nu of A (phi1's equation) and of B (phi2's)
  double lambda1[2][CVH_MAX_CHANNELS], lambda2[2][CVH_MAX_CHANNELS];
  CvhFrontArgs f;
  double stop[2];                              // what cvh_get_stop_condition returns for A and for B
  // what the table form alone reads, behind everything the by-value form shares with it (whose kernel arguments stay laid out as they were)
  CvhMpState *st_mirror;           // the pair's slot of the leader's contiguous state table: what the host reads, ONE copy for all members
  unsigned first;                  // workgroups of the step grid in front of this member's
};
// tab[0 .. nmem-1]: the members of ONE (channel count, math mode) class; grid: the sum of their step grids.  one (a HOST record,
// first = 0) non-null: the call has one member, whose record travels by value instead -- the single calls' launch
hipError_t cvh_launch_mp_sums(const CvhMpArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhMpArgs *one);   // the sums of u[.][parity] into partials
hipError_t cvh_launch_mp_step(const CvhMpArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhMpArgs *one);   // one iteration, and the sums of what it wrote
hipError_t cvh_launch_mp_finalize(const CvhMpArgs *tab, int nmem, int channels, int is_init, hipStream_t s, const CvhMpArgs *one);                      // a workgroup per member
// labels: one member; src phi1, src2 phi2, dst the bytes (any alignment), sections of cvh_io_blocks(n) workgroups
hipError_t cvh_launch_mp_labels(const CvhIoMember *tab, int nmem, unsigned grid, hipStream_t s);
// localised regions (localized_kernels.hip; include/chanvese_hip.h, "Localised regions").  Per iteration a ROW pass (a workgroup per row
// segment of CVH_WINDOW_SEGMENT columns) writes the horizontal window sums of wq and wq f_k -- 1 + C planes of unsigned 64-bit integers
// -- into the context's workspace; a STEP kernel's waves march down strips of strip_rows rows x CVH_MARCH_COLS columns with the vertical
// running sums of those planes in registers.  ||d||^2 is stored per ITEM -- item_rows rows x CVH_MARCH_COLS columns, a function of the
// shape alone; a strip is a whole number of items, that number a function of the radius -- and added by the one-workgroup finalise.
#define CVH_LOC_RADIUS_MAX 127
#define CVH_LOC_FRAC_BITS 40     // wq = rint(H_eps 2^40)
#define CVH_LOC_LEAD 2           // a strip has at least CVH_LOC_LEAD (2 R + 1) rows: its lead-in is at most a third of the workspace rows it reads
static_assert((2ull * CVH_LOC_RADIUS_MAX + 1) * (2 * CVH_LOC_RADIUS_MAX + 1) * 255 < (1ull << (64 - CVH_LOC_FRAC_BITS)),
              "every window sum fits in 64 unsigned bits: 65025 * 255 * 2^40 < 2^64");
struct CvhLocGeom { int nwc, item_rows, nitem_rows, nitems, strip_rows, nstrips, nseg; unsigned grid, row_grid; };
CvhLocGeom cvh_loc_geometry(int h, int w, int radius);
struct CvhLocState {
  CvhMarchCount run;
  double norm;                     // ||d||_2 of the last executed iteration
};
// A member of a localised launch: a record of the device table the kernels read (as CvhMpArgs above).  row_first / wave_first: the
// prefix block counts of the row pass's and the wave kernel's grids.  A launch of parity p reads u[p] and (step) writes u[p ^ 1].
struct CvhLocArgs {
  double *u[2];                    // both buffers of the level set
  const uint8_t *img[CVH_MAX_CHANNELS];
  CvhLocState *st;                 // the member's own state block (its workspace)
  double *partials;                // [nitems]
  unsigned long long *hw;          // [1 + C][h][w]: horizontal window sums of wq, wq f_k (plane-sum pass: of 1, f_k)
  unsigned *tsum;                  // [C][h][w]: T_k, the window sums of f_k
  double *trace;                   // [trace_cap] or null
  int trace_cap;
  int h, w, radius;
  CvhLocGeom g;
  double alpha, beta, gamma;       // dt mu, dt / C, -dt nu
  double lambda1[CVH_MAX_CHANNELS], lambda2[CVH_MAX_CHANNELS];
  CvhFrontArgs f;
  double stop;                     // what cvh_get_stop_condition returns
  // cvh_localized_means: device planes or null
  unsigned long long *wq_out, *a_out, *s_out;
  double *c1_out, *c2_out;
  // what the table form alone reads, behind everything the by-value form shares with it (whose kernel arguments stay laid out as they were)
  CvhLocState *st_mirror;          // the member's slot of the leader's contiguous state table: what the host reads, ONE copy for all members
  unsigned row_first, wave_first;  // workgroups of the row pass's / the wave kernel's grid in front of this member's
};
enum { CVH_LOC_STEP = 0, CVH_LOC_MEANS = 1, CVH_LOC_TSUM = 2 };
// tab[0 .. nmem-1]: the members of ONE (channel count, math mode) class; grid: the sum of their grids of that kernel.
// The row pass that goes with the wave kernel of kind `pass`: STEP reads the run's stop flag, MEANS does not, TSUM has wq = 1 (the plane sums)
// one (a HOST record, row_first = wave_first = 0) non-null: the call has one member, whose record travels by value instead (as above)
hipError_t cvh_launch_loc_rows(const CvhLocArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, int pass, hipStream_t s, const CvhLocArgs *one);
hipError_t cvh_launch_loc_wave(const CvhLocArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, int kind, hipStream_t s, const CvhLocArgs *one);
hipError_t cvh_launch_loc_finalize(const CvhLocArgs *tab, int nmem, hipStream_t s, const CvhLocArgs *one);   // a workgroup per member
// edge-weighted length (geodesic_kernels.hip, edge_kernels.hip; include/chanvese_hip.h, "Edge-weighted length").  ONE level set with
// global means on the four-phase partition (cvh_mp_geometry: the items are strips of strip_rows rows x CVH_MARCH_COLS columns).  An
// item's row of partial sums holds cvh_geo_nsums(C) doubles:  [0] sum H   [1 + k] sum I_k H   [1 + C] sum d^2.  The complements come
// from npix and sum_img, which do not depend on the level set: c2 = (sum I_k - sum I_k H) / (npix - sum H).
#define CVH_EDGE_ONE 32768       // gq of g = 1: g = gq 2^-15
__host__ __device__ constexpr int cvh_geo_nsums(int C) { return 2 + C; }
struct CvhGeoState {
  CvhMarchCount run;
  double c1[CVH_MAX_CHANNELS], c2[CVH_MAX_CHANNELS];   // the means of the current level set, read by the next iteration
  double norm;                     // ||d||_2 of the last executed iteration
};
// A member of a geodesic launch: a record of the device table the kernels read (as CvhMpArgs above)
struct CvhGeoArgs {
  double *u[2];                    // both buffers of the level set (by value: u[0] read, u[1] written)
  const uint8_t *img[CVH_MAX_CHANNELS];
  const uint16_t *gq;              // the edge plane
  CvhGeoState *st;                 // the member's own state block (its workspace)
  double *partials;                // [nitems][cvh_geo_nsums(C)]
  double *trace;                   // [trace_cap][2C + 1] or null
  int trace_cap;
  int h, w;
  CvhMpGeom g;
  double alpha, beta, gamma;       // dt mu, dt / C, -dt nu
  double lambda1[CVH_MAX_CHANNELS], lambda2[CVH_MAX_CHANNELS];
  CvhFrontArgs f;
  double stop;                     // what cvh_get_stop_condition returns
  double npix, sum_img[CVH_MAX_CHANNELS];   // h w and the exact plane sums
  // what the table form alone reads
  CvhGeoState *st_mirror;          // the member's slot of the leader's contiguous state table
  unsigned first;                  // workgroups of the step grid in front of this member's
};
// as the four-phase launchers: tab[0 .. nmem-1] the members of ONE (channel count, math mode) class, `one` a host record that travels by value
hipError_t cvh_launch_geo_sums(const CvhGeoArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhGeoArgs *one);
hipError_t cvh_launch_geo_step(const CvhGeoArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhGeoArgs *one);
hipError_t cvh_launch_geo_finalize(const CvhGeoArgs *tab, int nmem, int channels, int is_init, hipStream_t s, const CvhGeoArgs *one);
// convex relaxation (convex_kernels.hip; include/chanvese_hip.h, "Convex relaxation").  The primal-dual iteration of the relaxed
// two-phase model on the four-phase partition (cvh_mp_geometry).  The relaxation state of a context lives in its workspace:
//   [state block][the items' rows of partial sums][v][vbar 0][qx 0][qy 0][vbar 1][qx 1][qy 1]      -- 7 planes of h w doubles, 56 bytes per pixel
// v is updated in place (an iteration reads it at the pixel's own place alone); vbar, qx and qy are double-buffered, because a wave
// recomputes the dual of its halo column and of the row above its strip from the OLD values.  An item's row of partial sums holds
// cvh_cvx_nsums(C) doubles:  [0] sum v'   [1 + k] sum I_k v'   [1 + C] sum d^2.
__host__ __device__ constexpr int cvh_cvx_nsums(int C) { return 2 + C; }
struct CvhCvxState {
  CvhMarchCount run;
  double c1[CVH_MAX_CHANNELS], c2[CVH_MAX_CHANNELS];   // the means the next iteration uses
  double norm;                     // ||d||_2 of the last executed iteration
  int since, pad;                  // iterations since the means were last retaken: kept across calls (resume)
};
struct CvhCvxBufs { double *vbar, *qx, *qy; };   // one set of the double-buffered planes
// A member of a convex launch: a record of the device table the kernels read (as CvhMpArgs above)
struct CvhCvxArgs {
  CvhCvxBufs u[2];                 // both sets (by value: u[0] read, u[1] written); the start launch writes u[0]
  double *v;                       // updated in place
  const double *levelset;          // the start launch: the level set whose mask v0 is
  const uint8_t *img[CVH_MAX_CHANNELS];
  const uint16_t *gq;              // the edge plane, or null: g = 1
  CvhCvxState *st;                 // the member's own state block (its workspace)
  double *partials;                // [nitems][cvh_cvx_nsums(C)]
  double *trace;                   // [trace_cap][2C + 1] or null
  int trace_cap;
  int h, w;
  CvhMpGeom g;
  double tau, sigma, mu, nu;
  double lambda1[CVH_MAX_CHANNELS], lambda2[CVH_MAX_CHANNELS];
  double stop;                     // stop_rms sqrt(h w), taken once on the host; negative: no rule
  double npix, sum_img[CVH_MAX_CHANNELS];   // h w and the exact plane sums
  int means_every, resume;
  // what the table form alone reads
  CvhCvxState *st_mirror;          // the member's slot of the leader's contiguous state table
  unsigned first;                  // workgroups of the step grid in front of this member's
};
// as the four-phase launchers: tab[0 .. nmem-1] the members of ONE (channel count, math mode) class, `one` a host record that travels by
// value.  start: v0, vbar0 = v0, q = 0 into u[parity] and the sums of v0 (a member with `resume` returns at once); finalize with is_init:
// the whole state block from those sums, or -- a member with `resume` -- the run counters alone
hipError_t cvh_launch_cvx_start(const CvhCvxArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhCvxArgs *one);
hipError_t cvh_launch_cvx_step(const CvhCvxArgs *tab, int nmem, unsigned grid, int parity, int channels, int fast, hipStream_t s, const CvhCvxArgs *one);
hipError_t cvh_launch_cvx_finalize(const CvhCvxArgs *tab, int nmem, int channels, int is_init, hipStream_t s, const CvhCvxArgs *one);
hipError_t cvh_launch_cvx_bake(const double *v, double *u, size_t n, hipStream_t s);   // u = v - 0.5
// the Sobel edge map (edge_kernels.hip) on the member table: src / src_stride / w2 the planes of the source context and their number,
// dst the member's edge plane (uint16), den[i] member i's ((64 C) K) K, a table behind the member table; a lane takes a pixel per trip,
// sections of cvh_edge_blocks(n) workgroups.  The device-pointer forms: a clamped copy in, a plain copy out.
unsigned cvh_edge_blocks(size_t n);
hipError_t cvh_launch_edge_map(const CvhIoMember *tab, const double *den, int nmem, unsigned grid, hipStream_t s);
hipError_t cvh_launch_edge_clamp(const uint16_t *src, uint16_t *dst, size_t n, hipStream_t s);   // dst = min(src, CVH_EDGE_ONE)
// rows-per-tile options of the step kernel
void cvh_step_grid(int h, int w, int tile_rows, int *tiles_x, int *tiles_y);
int cvh_step_max_blocks(int h, int w);
hipError_t cvh_launch_step(const CvhStepArgs &a, int channels, int fast, hipStream_t s);
int cvh_wave2_cols();
// batch non-null: the same instantiation's batch entry point over a fused grid (a = any member's arguments: selects the flavour)
hipError_t cvh_launch_wave2(const CvhStepArgs &a, int channels, int fast, hipStream_t s, const CvhBatchLaunch *batch = nullptr);
// one-buffer flow (csv_wave2_kernel.hip): dense plane -> slab with the pads and shadow rows of parity `par`; slab -> dense plane
hipError_t cvh_launch_ob_pack(const double *dense, double *slab, const int *tab, int h, int w, int nwc, int nstrips, int par, hipStream_t s);
hipError_t cvh_launch_ob_unpack(const double *slab, double *dense, int h, int w, int nwc, hipStream_t s);
hipError_t cvh_launch_chain_flush(const CvhStepArgs &a, int channels, hipStream_t s);
size_t cvh_pm_resident_lds_bytes();
int cvh_pm_resident_halo_doubles();
int cvh_pm_resident_blocks_per_cu();
hipError_t cvh_launch_pm_resident(const CvhPmArgs &a, hipStream_t s);
int cvh_pm_resident_batch_blocks_per_cu();
hipError_t cvh_launch_pm_resident_batch(const CvhPmBatchArgs &b, int fast, int nr, hipStream_t s, CvhLaunchNote *note = nullptr);
hipError_t cvh_launch_pm_load_batch(const CvhPmIoPlane *planes, int nplanes, size_t nmax, hipStream_t s);
hipError_t cvh_launch_pm_store_batch(const CvhPmIoPlane *planes, int nplanes, size_t nmax, hipStream_t s);
size_t cvh_resident_lds_bytes(int channels);
int cvh_resident_tile_w();
int cvh_resident_tile_hmax(int channels);   // most rows of a tile: 128 for one channel, 96 for three (three image tiles and tables in LDS)
int cvh_resident_halo_doubles();
int cvh_resident_blocks_per_cu(int channels);
hipError_t cvh_launch_resident(const CvhStepArgs &a, int channels, hipStream_t s);   // cooperative launch, a.res_steps iterations in LDS
hipError_t cvh_launch_wave(const CvhStepArgs &a, int channels, int fast, hipStream_t s, const CvhBatchLaunch *batch = nullptr);
int cvh_wave_cols();
hipError_t cvh_launch_init_sums(const CvhStepArgs &a, int channels, int fast, int *nparts_out,
                                hipStream_t s);
hipError_t cvh_launch_finalize(const CvhStepArgs &a, int channels, int is_init, hipStream_t s);
int cvh_init_sum_blocks(int h, int w);

hipError_t cvh_launch_pm_load(const uint8_t *plane, double *state, size_t n, hipStream_t s);
hipError_t cvh_launch_pm_step(const CvhPmArgs &a, hipStream_t s);
hipError_t cvh_launch_pm_wave(const CvhPmArgs &a, hipStream_t s);
int cvh_pm_wave_k2_cols();
hipError_t cvh_launch_pm_wave_k2(const CvhPmArgs &a, hipStream_t s);   // TWO time steps per launch
int cvh_pm_wave_cols();
hipError_t cvh_launch_pm_store(const double *state, uint8_t *plane, size_t n, hipStream_t s);
void cvh_pm_grid(int h, int w, int *tiles_x, int *tiles_y);

hipError_t cvh_launch_contour(const double *u, uint8_t *out, int h, int w, hipStream_t s);
hipError_t cvh_launch_state_narrow(double *u, float *uf, size_t n, hipStream_t s);       // uf = (float)u, u = (double)uf
hipError_t cvh_launch_state_widen(const float *uf, double *u, size_t n, hipStream_t s);  // u = (double)uf
hipError_t cvh_launch_ppf(double *data, size_t n, int op, double eps, hipStream_t s);
hipError_t cvh_launch_separate(const uint8_t *img3, const double *u, uint8_t *sel3, size_t n,
                               int invert, hipStream_t s);
