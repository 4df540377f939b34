/*
 * chanvese_hip.h — C ABI of the MI355X-native Chan-Sandberg-Vese / Perona-Malik hot path.
 *
 * This is the drop-in boundary for ktht/chan_vese: plain C, opaque context, caller-owned
 * host buffers, library-owned device buffers, one HIP stream per context, no exceptions
 * across the boundary (every entry point returns a cvh_status; cvh_last_error() gives the
 * text).  Each entry point names the reference code it replaces (file:line relative to
 * the reference repo).  The reference-side binding is shown in INTEGRATION.md.
 *
 * Layouts (identical to the reference): level set u = h*w IEEE doubles, row-major,
 * contiguous (src/main.cpp:225-227 treats u.data as double[h*w]); image channels = C
 * separate planes of h*w uint8, row-major (src/main.cpp:269-270, after cv::split :936).
 * Channel order is whatever the caller split (BGR for cv::imread colour, :879).
 *
 * Threading: calls on one context are not re-entrant; different contexts (different
 * images / GPUs) may be driven from different host threads.
 *  - A batch call counts as a call on every one of its members: no member may be in
 *    another call, on any thread, while the batch call runs.
 *  - cvh_last_error(NULL) is per thread: it returns the last context-less error (a failed
 *    cvh_create, a refused batch) of the calling thread.
 */
#ifndef CHANVESE_HIP_H
#define CHANVESE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVH_MAX_CHANNELS 3

typedef enum cvh_status {
  CVH_OK = 0,
  CVH_ERR_ARG = 1,    /* bad argument (null pointer, non-positive size, channels not 1/3 ...) */
  CVH_ERR_HIP = 2,    /* a HIP runtime call failed; see cvh_last_error() */
  CVH_ERR_STATE = 3,  /* call sequence error (e.g. run before set_image / set_levelset) */
  CVH_ERR_NOMEM = 4
} cvh_status;

/* Pixel functions the ParallelPixelFunction operator can run on the device.  The
 * reference passes an opaque std::function (include/ParallelPixelFunction.hpp:26-28);
 * its only use is delta_eps (src/main.cpp:988-989), the Heaviside pair is what
 * region_variance evaluates per pixel (src/main.cpp:265-267). */
typedef enum cvh_pixel_op {
  CVH_OP_DELTA = 0,               /* regularized_delta      src/main.cpp:204-210 */
  CVH_OP_HEAVISIDE = 1,           /* regularized_heaviside  src/main.cpp:188-194 */
  CVH_OP_ONE_MINUS_HEAVISIDE = 2  /* the Outside lambda     src/main.cpp:267     */
} cvh_pixel_op;

/* Arithmetic flavour of the fused level-set kernel (both keep FP64 state). */
typedef enum cvh_math_mode {
  CVH_MATH_DEFAULT = 0, /* library default */
  CVH_MATH_STRICT = 1,  /* IEEE sqrt and divide, no FMA contraction: every per-pixel
                           operation rounds as the reference's -O3 x86-64 code does; only
                           atan (device libm) and the summation order differ */
  CVH_MATH_FAST = 2     /* rsqrt/rcp + Newton, FMA: <= 2 ulp per operation */
} cvh_math_mode;

/* Free parameters of the CSV iteration: src/main.cpp:731-734, defaults :759-765,:812-829 */
typedef struct cvh_params {
  double mu;                        /* length penalty, default 0.5 */
  double nu;                        /* area penalty, default 0 */
  double dt;                        /* time step, default 1 */
  double eps;                       /* Heaviside/delta smoothing, default 1 */
  double tol;                       /* stop tolerance, default 0.001 */
  double lambda1[CVH_MAX_CHANNELS]; /* inside penalties, default 1 */
  double lambda2[CVH_MAX_CHANNELS]; /* outside penalties, default 1 */
} cvh_params;

typedef struct cvh_context cvh_context;

/* Fills *p with the reference defaults (src/main.cpp:759-765, :812-813, :828-829). */
void cvh_default_params(cvh_params *p);

/* Number of HIP devices visible to this process. */
int cvh_device_count(int *count);

/* Creates a context for one h x w image with `channels` (1 = -g grayscale path, 3 =
 * colour; src/main.cpp:893) on HIP device `device`.  Allocates the device planes, the
 * level-set ping-pong pair and the reduction workspace.  On failure *out is NULL and
 * cvh_last_error(NULL) describes why. */
int cvh_create(cvh_context **out, int h, int w, int channels, const cvh_params *p,
               int device);
void cvh_destroy(cvh_context *ctx);

/* Text of the last error on this context (or, when ctx is NULL, of the calling thread's last
 * context-less failure: a failed cvh_create, a refused batch).  Never NULL.  Replaces the reference's msg_exit text, src/main.cpp:173-178. */
const char *cvh_last_error(const cvh_context *ctx);

/* Replaces the parameter block (may be called between runs). */
int cvh_set_params(cvh_context *ctx, const cvh_params *p);

/* Tuning / behaviour knobs, by name (defaults are what bench.py measures):
 *   "math_mode"      cvh_math_mode
 *   "finalize"       0 = region means reduced by the last-arriving workgroup inside the step
 *                    kernel (default), 1 = by a separate one-workgroup kernel
 *   "trace"          capacity (iterations) of the per-iteration trace, 0 = off
 *   "sync_every"     iterations enqueued between host polls of the stop flag (default 32)
 *   "graph"          1 = runs of 16 steps are replayed as one hipGraph (default), 0 = plain launches
 *   "kernel"         data flow of the CSV step: -1 auto (3 where it applies -- width a multiple of 16 and >= 144, from 0.6 Mpixel; three
 *                    channels in FAST arithmetic only -- else 2; 0 from 2^28 pixels),
 *                    0 LDS tile, 2 wave-streaming, 3 wave-streaming with 2 pixels per lane (w % 16 == 0, w >= 144; other shapes
 *                    fall back to 2).  (1, the streaming-strip kernel of round 1, was removed in round 4: CVH_ERR_ARG)
 *   "resident"       -1 auto (default), 0 off, 1 on: planes whose level set fits the LDS of the chip (1 channel, FAST, even width,
 *                    at most one 128 x 128 tile per CU: up to 2048 x 2048 on an MI355X) iterate IN LDS -- one cooperative launch per
 *                    chunk of iterations, one workgroup per tile, a grid barrier per iteration, the stop rule inside the kernel at the
 *                    reference's iteration (csv_resident_kernel.hip).  Auto steps aside when "kernel", "strip_rows", "strips" or
 *                    "graph" were set (the caller asked for a per-launch flow), when "state" is 32, and -- enqueue by enqueue -- when
 *                    other co-resident contexts live on the device (a batch: cooperative launches of different contexts serialise, and
 *                    interleaved per-launch flows are twice as fast in short chunks) UNLESS the plane is large and the enqueue long:
 *                    from 48 iterations at >= 3.6 Mpixel, 72 at >= 2.9, 100 at >= 2.2 (cvh_run: chunks of up to 1024) one cooperative
 *                    launch after the other wins (eight 2048 x 2048 planes: 12.1-14.7 against 16.2 us per image-iteration).  The two
 *                    flows continue each other on one context and agree to 1e-9, not bit for bit: set 0 or 1 for the same bits
 *                    whatever the chunking
 *                    THREE CHANNELS take the resident flow on request only: 1 runs csv_resident_kernel<3, NRT> where the plane
 *                    qualifies under the same conditions (FAST, even width, "state" 64) with tiles of at most 96 rows -- the three
 *                    image tiles and region tables live in LDS beside the level set -- i.e. up to 256 tiles of 96 x 128: 1536 x 2048
 *                    (1080 x 1920 fits; 2048 x 2048 x 3 does not).  A plane that does not fit keeps the per-launch flow silently;
 *                    -1 (auto) keeps the per-launch flow for three channels.  Measured on an MI355X, resident against
 *                    per launch, us per iteration: 256 x 256 6.6 / 8.1, 512 x 512 6.9 / 9.3, 1024 x 1024 8.3 / 13.4, 1080 x 1920
 *                    11.9 / 17.8, 1536 x 2048 14.4 / 21.0 -- 1 pays at every three-channel size that fits, for a context that runs
 *                    alone on its GPU (cooperative launches of different contexts serialise, as with one channel)
 *   "wave_pol"       cache policy of the streamed level-set rows: -1 auto (write-through stores while the ping-pong pairs and planes of
 *                    ALL contexts on the device that hold an image and a level set fit the Infinity Cache, <= 300 MB together; decided
 *                    when a run's first iteration is enqueued, kept for the run), 0 plain, 1 write-through
 *   "co_resident"    1 (default): this context streams beside the others on its GPU and counts in their automatic choices ("wave_pol",
 *                    "resident"); 0: a scratch / warm-up context that is idle while the others run.  The levels of a pyramid
 *                    ("Coarse-to-fine" below) never stream beside each other: while one level runs, a driver sets 0 on the
 *                    pyramid's other levels, and on return the finest level has the value it had before and the helper levels
 *                    stay 0 -- the finest level then makes the choices it makes without a pyramid
 *   "state"          64 (default): the level set lives in HBM as double -- the reference's CV_64FC1 (src/main.cpp:225), the parity mode.
 *                    32: a DECLARED fast mode that deliberately departs from the reference's type: float in HBM (9 instead of 17 bytes
 *                    per pixel-iteration; 11 instead of 19 with three channels), every new value rounded to float; arithmetic, tables
 *                    and the fixed-point sums unchanged.  2-pixel wave kernel only: FAST arithmetic, width a multiple of 16 and >= 144,
 *                    fewer than 2^28 pixels (CVH_ERR_ARG otherwise).  cvh_set_levelset / cvh_get_levelset keep exchanging doubles.
 *                    Parity bar: mask IoU >= 0.999 and median |du| / max|u| <= 1e-4 against the FP64 path
 *   "near_switch"    1 (default): a wave whose strip / band starts where most pixels are below the far-field threshold of H_eps (32 eps)
 *                    evaluates the table form of H_eps on every pixel of that strip (one form per pixel: a level set that is near
 *                    everywhere, e.g. dt << 1); 0: the far-field series with the per-group correction everywhere
 *   "one_buffer"     2-pixel wave kernel, one channel, FAST arithmetic, FP64 state, a context's own launches of a run that cannot stop
 *                    (tol == 0): the iterations update ONE padded level-set buffer in place instead of the ping-pong pair; what a wave
 *                    reads of its neighbours comes from row pads and shadow rows, double-buffered by iteration parity.
 *                    -1 (default): automatic -- a single live context whose pair (with the image) exceeds what the 256 MiB Infinity
 *                    Cache holds while one buffer fits (4096^2: 285 against 160 MB), in the automatic geometry ("kernel", "strip_rows",
 *                    "strips" and the strip skews untouched); 0: the pair; 1: one buffer wherever the flow
 *                    exists.  The results are the same bit for bit (tests/test_gpu_one_buffer.py).  Every caller of the level set
 *                    (get, mask, set, the device-side calls) sees the dense plane: the padded buffer is converted on demand.
 *   "wave_seam"      2-pixel wave kernel, FAST arithmetic: 1 (default): the final group of a strip requests and parks no rows, east
 *                    extra or image pieces of a group that does not exist; 0: it does, like every other group.  The results are the
 *                    same bit for bit (tests/test_gpu_wave2_seam.py); the key exists for that comparison.  (The name is the seam of a
 *                    workgroup's two strips: handing its rows over in LDS is the part that does not ship)
 *   "tile_rows"      tile kernel: rows per tile (0 auto, 14/16)
 *   "strip_rows"     wave kernels: rows per strip (0 auto)
 *   "lut"            1 = region term from a per-launch 256-entry table (FAST, default; tile and 1-pixel wave kernels: 0 = computed)
 *   "dma"            tile kernel: 1 = global->LDS DMA loader (slower on MI355X, default 0)
 *   "pm_kernel"      Perona-Malik data flow: -1 auto (= 4 where the plane qualifies, else 3), 0 LDS tile,
 *                    1 wave-streaming, 3 wave-streaming with TWO time steps per launch (an odd last step runs flavour 1),
 *                    (2, a 2-pixel-per-lane 1-step kernel, was removed in round 4: CVH_ERR_ARG)
 *                    4 resident plane: the FP64 state of a channel stays in the LDS of the CUs for all time steps, one
 *                    cooperative launch per channel (even width, >= 16 rows and columns, <= 128 rows x 128 columns per CU:
 *                    up to 2048 x 2048 on MI355X; CVH_ERR_ARG if asked for a plane that does not qualify; auto steps
 *                    aside when "pm_strip_rows" was set)
 *   "pm_strip_rows"  Perona-Malik wave kernel: rows per strip (0 auto)
 * (Ablation / diagnostic knobs of the wave kernels are not part of this interface: they are listed in
 * chan_vese_amd/csrc/cvh_internal.h.)  Unknown keys and out-of-range values return CVH_ERR_ARG. */
int cvh_set_option(cvh_context *ctx, const char *key, long value);

/* Uploads the C channel planes (what cv::split produced, src/main.cpp:934-937) and takes their sums on the device
 * (sum I_k for the region means; the tol-free stop norm of :950-959 — exact integers for one channel, the reference's
 * serial order on the host for three). */
int cvh_set_image(cvh_context *ctx, const uint8_t *const *planes);
/* Downloads the planes (after cvh_perona_malik they hold the smoothed 8-bit image that
 * the reference writes as <stem>_pm, src/main.cpp:943-946). */
int cvh_get_image(cvh_context *ctx, uint8_t *const *planes);

/* Level set in / out (src/main.cpp:898-923 produce it, :1004-1005 consume it). */
int cvh_set_levelset(cvh_context *ctx, const double *u);
int cvh_get_levelset(cvh_context *ctx, double *u);
/* levelset_checkerboard, src/main.cpp:221-233.  The h + w sine factors are evaluated on the HOST
 * with libm sin (the sign on every fifth row/column is rounding noise that only the host libm
 * reproduces) and uploaded; the sign of their product — one IEEE multiplication — is taken on the
 * device, bit-identical to cvh_levelset_checkerboard_host without 8 bytes per pixel over PCIe.
 * cvh_init_checkerboard_batch of this one context: one launch, one host wait. */
int cvh_init_checkerboard(cvh_context *ctx);
/* Host-only helper with the same arithmetic, for callers that keep u themselves. */
void cvh_levelset_checkerboard_host(int h, int w, double *u);

/* The timestep loop, src/main.cpp:963-1001: runs until `max_steps` further iterations
 * are done or the stop rule ||u_diff||_2 <= tol*||mean_k I_k||_2 fires (checked after the
 * update, :994-1000).  max_steps < 0 means unlimited (:890).  steps_done / last_norm
 * (may be NULL) receive the iterations executed by this call and the last ||u_diff||_2.
 * One fused HIP kernel per iteration: curvature (:342-375), region terms (:255-312,
 * :965-985), delta_eps map (ParallelPixelFunction, :988-992), update and norm (:993-994),
 * plus the Heaviside-weighted sums that give the next iteration's c1/c2 (:973-974). */
int cvh_run(cvh_context *ctx, int max_steps, int *steps_done, double *last_norm);

/* Asynchronous halves of cvh_run, for interleaving several contexts (a batch of
 * independent images) on one GPU: enqueue `nsteps` iterations on the context's stream,
 * later wait for them.  `stopped` reports whether the stop rule fired. */
int cvh_enqueue_steps(cvh_context *ctx, int nsteps);
/* Optional: does the one-off host work of an upcoming cvh_enqueue_steps(ctx, nsteps) now (strip table,
 * capture + instantiation of the 16-step hipGraph of the position the chunk starts at), so that a caller
 * timing the enqueue/sync pair with its own clock does not see it.  cvh_run and cvh_enqueue_steps do the
 * same work themselves before they open cvh_last_run_ms's interval. */
int cvh_warm(cvh_context *ctx, int nsteps);
int cvh_sync(cvh_context *ctx, int *steps_done_total, double *last_norm, int *stopped);
/* Clears the iteration counter and the stop flag (cvh_run does this itself). */
int cvh_reset_run(cvh_context *ctx);

/* Fused batch: n contexts on one device advance together, with ONE kernel launch per iteration for all members that share
 * a CSV-step instantiation (the kernel= text of cvh_launch_info; a batch of one shape is one launch).  Per member it is
 * exactly what its own calls do -- src/main.cpp:963-1001, its own stop rule, trace, sums and level set; the members'
 * bits are those of their own per-launch runs on the same strips.  Everything else stays per context (cvh_set_image,
 * cvh_get_*, cvh_sync, cvh_perona_malik), and a context may alternate between its own runs and batch runs at any
 * enqueue boundary.
 *   cvh_enqueue_steps_batch: enqueues nsteps iterations of every member; then cvh_sync each member, as after
 *     cvh_enqueue_steps.
 *   cvh_run_batch: cvh_run per member -- resets every member's run; each stops at its own reference iteration (:1000)
 *     and the batch's later iterations are no-ops for it; ends when every member has stopped or max_steps iterations
 *     are done; steps_done[i] / last_norm[i] (arrays of n, or NULL) as cvh_run's.
 * Members always take the per-launch wave kernels (never the resident flow).  The automatic strip count of a member whose
 * own strips are short (below 32 rows: planes up to ~2048^2 on MI355X) is sized for its share of the chip, num_cus x (its
 * pixels) / (all members' pixels); larger members keep their own geometry; an explicit "strip_rows" or "strips" wins.
 * The fused launches run on member 0's stream, ordered after everything already enqueued on every member's stream and
 * before anything enqueued on them later; cvh_last_run_ms of every member reports the fused interval.
 * Throughput: the fused batch pays off for small and mid-size planes (MI355X, us per image-iteration against the same
 * contexts interleaved: 64 x 256^2 about 2x, 32 x 512^2 1.4-1.7x, 8 x 1024^2 1.1-1.2x).  For large planes it is NOT
 * faster and can be a few per cent slower (8 x 4096^2): every fused iteration ends with the tail of its last workgroups,
 * which interleaved streams hide under the next iteration.  For planes of 2048^2 and more, interleave cvh_enqueue_steps.
 * The enqueue can block the host: it synchronises the leader's stream when the batch's argument tables must be re-uploaded
 * (first call, a change of members, options or geometry) and a member's stream when its strip table changes -- e.g. on
 * every switch of a context between its own runs and batch runs of another geometry.
 * CVH_ERR_ARG: ctxs NULL, n < 1, a NULL or duplicate member, members on different devices, a member with "finalize"
 * = 1 or one that takes the tile kernel (>= 2^28 pixels); CVH_ERR_STATE: a member without an image or a level set.
 * The message names the member index; it is cvh_last_error(NULL)'s and member 0's; the members stay usable. */
int cvh_enqueue_steps_batch(cvh_context *const *ctxs, int n, int nsteps);
int cvh_run_batch(cvh_context *const *ctxs, int n, int max_steps, int *steps_done, double *last_norm);

/* Region means of the current level set (what the next iteration will use),
 * region_variance src/main.cpp:255-281; c1/c2 have `channels` entries.
 * A region that holds no pixel still has a mean: the H_eps-weighted mean of the far tails eps/(pi |u|) of all pixels.
 * While every region holds a pixel (any |u|/eps up to 1e12, tests/test_gpu_lopsided.py) c1/c2 agree with the reference
 * to 1e-9.  With NO pixel on one side the reference itself defines that side's mean only to 2e-11 at |u|/eps = 1e7,
 * 1.5e-9 at 1e9 and 2.4e-6 at 1e12 (cancellation in 1 + 2/pi atan); the flavours with centred sums (FAST wave kernels,
 * resident, FP32 state, fused batch) are then within 6e-9, 4e-7 and 5.1e-4 of the accurate value;
 * the other side's mean, the level set and the norm keep their 1e-9.  From |u|/eps ~ 1e16 the empty side's mean is 0/0:
 * NaN here as in the reference, and from the iteration that used it on the level set, the norm and both means are NaN. */
int cvh_get_means(cvh_context *ctx, double *c1, double *c2);
/* Per-iteration trace rows [c1_0..c1_{C-1}, c2_0..c2_{C-1}, norm] recorded when the
 * "trace" option is on; *rows receives the number of valid rows copied (<= max_rows).
 * c1/c2 of a row are the means the iteration used: see cvh_get_means for empty regions and NaN. */
int cvh_get_trace(cvh_context *ctx, double *out, int max_rows, int *rows);
/* tol * || (sum_k I_k)/C ||_2, src/main.cpp:950-959 (valid after set_image). */
int cvh_get_stop_condition(cvh_context *ctx, double *stop_cond);

/* mask = ((float)u > 0), optionally 1 - mask: src/main.cpp:395-400.  cvh_get_mask_device of the context's own buffer, then copied
 * down: iterations enqueued and never synchronised are settled first, as every device-memory getter and cvh_get_mask_clean do (the mask
 * is that of the level set behind them; a later cvh_sync reports them as done). */
int cvh_get_mask(cvh_context *ctx, uint8_t *mask, int invert);
/* Contour map of the reference's video frame, VideoWriterManager::draw_contour
 * src/VideoWriterManager.cpp:60-74: 1 where a frame pixel is painted in the contour colour.
 * The frame's mask rule differs from cvh_get_mask: uint8(round(u)) > 0.
 * cv::findContours/drawContours are restated (see misc_kernels.hip); parity unpinned. */
int cvh_get_contour(cvh_context *ctx, uint8_t *contour);
/* separate(), src/main.cpp:386-405: img3 and selection3 are interleaved h*w*3 uint8
 * (the reference's CV_8UC3); white canvas with img3 copied where the mask is set. */
int cvh_separate(cvh_context *ctx, const uint8_t *img3, int invert, uint8_t *selection3);

/* perona_malik, src/main.cpp:478-560, applied in place to every device plane:
 * trip count from `for (double t = 0; t < T; t += L)` (:498), FP64 state, final
 * round-half-even to uint8 (:551).  Invalidates the stop condition (recomputed from the
 * smoothed planes, :950). */
int cvh_perona_malik(cvh_context *ctx, double K, double L, double T);
/* Trip count of that loop (host arithmetic). */
int cvh_pm_trip_count(double L, double T);

/* Perona-Malik batch: cvh_perona_malik(ctxs[i], K[i], L[i], T[i]) for n contexts on one device (K, L, T: arrays of n), with
 * the planes of several members sharing one cooperative launch of the resident kernel.  Per member it does exactly what its
 * own call does: every channel plane smoothed in place, byte for byte the planes of its own cvh_perona_malik; the stop
 * condition and the sums invalidated; synchronous.  A Perona-Malik step has no global sum, so a tile waits only for the
 * tiles of its own plane, and planes with different K, L and step counts share a launch (each plane's tiles leave after
 * its own steps).
 * A member is FUSED when its "pm_kernel" is -1 or 4, its "pm_strip_rows" is 0, its plane qualifies for the resident kernel
 * on its own (even width, >= 16 rows and columns, fits the chip's LDS) and its trip count is <= 65536.  Unlike one context's
 * automatic choice there is no minimum trip count: the launch cost is shared.  Every other member runs its own
 * cvh_perona_malik flow inside the same call.
 * Packing, deterministic: a C-channel member contributes C planes, channel k to round k; a round's FAST planes, then its
 * STRICT planes; first fit in member order into launches of at most min(resident workgroups the device holds, 256, CUs)
 * tiles; a launch takes the shortest band, 8 x {2, 4, 8, 16} rows per tile, at which all its planes' tiles fit together.
 * Each launch is one uint8 -> FP64 load, one resident launch and one FP64 -> uint8 store for all its planes.
 * All launches run on member 0's stream (after everything already enqueued on every fused member's stream) with member
 * 0's border buffer and error word; cvh_last_pm_ms of a fused member reports the batch's device interval, and
 * cvh_launch_info(ctx, 1) describes the fused launch of its first plane, with batch_planes= (planes in that launch) and
 * batch_launches= (fused launches of the call).
 * When it pays (MI355X, 400 steps, us per image-step against the per-context sequence): 64 x 256^2 22.6x (one launch of
 * 64 planes), 32 x 512^2 6.3x, 16 x 512^2 x 3 channels 6.2x, 8 x 1024^2 2.1x; 4 x 2048^2 1.03x -- a 2048^2 plane fills the
 * chip alone, so such members share only the launch overheads.  No measured size was slower.
 * CVH_ERR_ARG: ctxs NULL, n < 1, a NULL or duplicate member, members on different devices, K / L / T NULL, a member whose
 * L, T or K cvh_perona_malik refuses, "pm_kernel" = 4 on a plane that does not qualify; CVH_ERR_STATE: a member without an
 * image.  Checked for every member before anything runs (the planes stay untouched); the message names the member index
 * and is cvh_last_error(NULL)'s and member 0's.  CVH_ERR_HIP when a wait of the resident kernel gave up: every member's
 * planes are undefined. */
int cvh_perona_malik_batch(cvh_context *const *ctxs, int n, const double *K, const double *L, const double *T);

/* Device time (HIP events on the context's stream) of the last cvh_run / of the span
 * from the first cvh_enqueue_steps after a cvh_sync to that next cvh_sync; and of the
 * last cvh_perona_malik. */
int cvh_last_run_ms(cvh_context *ctx, float *ms);
int cvh_last_pm_ms(cvh_context *ctx, float *ms);
/* Which kernel the library launches, as "key=value" text written by the launch sites themselves (no counterpart in
 * the reference: the kernel is an implementation detail; bench.py names it in its roofline object and profiles/ are
 * matched against it).  phase 0: the CSV step as the next cvh_run / cvh_enqueue_steps launches it with the current
 * options -- kernel=<instantiation as rocprofv3 prints it> grid= block= lds_bytes= strips= strip_rows= chain= wave_pol=
 * math= steps_per_graph= wave_seam= one_buffer=; phase 1: what the last cvh_perona_malik launched (CVH_ERR_STATE before the first).
 * Launches nothing.  Truncates to cap - 1 characters. */
int cvh_launch_info(cvh_context *ctx, int phase, char *buf, int cap);

/* ParallelPixelFunction::operator()(cv::Range(start,end)) with a tagged function,
 * src/ParallelPixelFunction.cpp:12-17 — host buffer form: data is a w-wide CV_64FC1
 * matrix, elements [start,end) of its flat index range are replaced by f(x) in place
 * (copied to the device, mapped by a HIP kernel, copied back). */
int cvh_ppf_apply(double *data, int w, long start, long end, int op, double eps,
                  int device);
/* Same on a device pointer the caller owns (hip stream as void*, NULL = default). */
int cvh_ppf_apply_device(double *d_data, long n, int op, double eps, void *stream);

/* ---- Device-memory input and output -----------------------------------------------------------------------------------------
 * The calls above move CALLER-OWNED HOST buffers over PCIe and synchronise the context's stream, one context per call.  The calls
 * below take memory the caller owns ON THE DEVICE of the context(s) -- device, managed or mapped host memory, checked with
 * hipPointerGetAttributes -- and are ordered against the caller's HIP stream `stream` (as void *, NULL = the default stream):
 *   inputs   an event is recorded on `stream` when the call is made and the library's stream waits for it: whatever the caller
 *            enqueued on `stream` before the call is read complete;
 *   outputs  an event is recorded behind the library's last launch and `stream` waits for it: work the caller enqueues on `stream`
 *            after the call sees the result.  The library never synchronises the caller's stream on the host, and an output call does
 *            not wait for its own work.  It can still block the host in three cases: the context has iterations in flight (enqueued,
 *            not yet cvh_sync'ed) or "state" = 32 needs its double mirror refreshed -- those are settled first, as the host-buffer
 *            getters do --; and every call that launches a kernel writes its member table into one pinned block of the leading
 *            context, so it first waits until the PREVIOUS such call led by that context has run.  That is long past in a frame loop
 *            that consumes its masks, but a second output call issued while the first is still queued behind the caller's stream
 *            waits for that stream's work.
 * The *_batch forms serve n contexts of one device with ONE kernel launch on member 0's stream, joined with every member's stream
 * before and after (as cvh_enqueue_steps_batch); the single-context forms are the same kernels with n = 1.
 * Results are those of the host-buffer calls, bit for bit: cvh_set_image_device leaves the planes, the sums, the stop norm and the
 * validity flags of cvh_set_image of the same bytes; cvh_set_levelset_device those of cvh_set_levelset (bits = 32 takes floats and is
 * cvh_set_levelset of their exact double values); cvh_get_levelset_device with bits = 32 rounds to nearest even.
 * Layouts: CVH_LAYOUT_PLANAR is C planes of h*w bytes one behind the other (what cvh_set_image takes), CVH_LAYOUT_INTERLEAVED is
 * h*w*C bytes (the reference's CV_8UC3, what cv::split consumes at src/main.cpp:934-937).  uint8 pointers may have ANY byte
 * alignment; level-set pointers are aligned to their element.
 * Host waits: the ingest calls wait ONCE per call (the sums come back to host fields) where cvh_set_image waits once per context.
 * One channel is summed entirely on the device (exact integers).  THREE channels: (sum_k I_k)/3 is rounded per pixel and the
 * reference adds the squares serially, four per step, so the planes are fetched and summed on the host as cvh_set_image's route
 * does -- for all members of a batch behind the one wait, the members' sums on up to 16 host threads.  Cost of that fetch: 3 bytes
 * per pixel over PCIe plus the serial sum -- measured on an MI355X for 16 x 480 x 640 x 3: 0.93 ms of a 1.42 ms ingest (the same 48
 * planes as one-channel members: 0.49 ms; tools/device_io_probe.py).  cvh_init_checkerboard_batch and cvh_set_levelset_device wait once per call as well
 * ("state" = 64; with "state" = 32 every member's float pair then adopts the level set: one more launch and wait per member).
 * Buffers of different members that overlap each other are the caller's business: nothing checks it.
 * CVH_ERR_ARG: NULL pointers, n < 1, a NULL or duplicate member, members on different devices, an unknown layout, bits not 32 or
 * 64, a pointer that is not device-accessible memory of the context's device; CVH_ERR_STATE: a getter before an image / a level
 * set exists.  Checked for every member before anything is launched; a batch's message names the member index and is
 * cvh_last_error(NULL)'s and member 0's; the members stay usable. */
typedef enum cvh_layout { CVH_LAYOUT_PLANAR = 0, CVH_LAYOUT_INTERLEAVED = 1 } cvh_layout;

int cvh_set_image_device(cvh_context *ctx, const uint8_t *d_img, int layout, void *stream);
/* The planes as they are now (after cvh_perona_malik: the <stem>_pm image). */
int cvh_get_image_device(cvh_context *ctx, uint8_t *d_img, int layout, void *stream);
int cvh_set_levelset_device(cvh_context *ctx, const void *d_u, int bits, void *stream);
int cvh_get_levelset_device(cvh_context *ctx, void *d_u, int bits, void *stream);
/* mask = ((float)u > 0), optionally 1 - mask, h*w bytes. */
int cvh_get_mask_device(cvh_context *ctx, uint8_t *d_mask, int invert, void *stream);

int cvh_set_image_device_batch(cvh_context *const *ctxs, int n, const uint8_t *const *d_imgs, int layout, void *stream);
/* cvh_init_checkerboard for n contexts: the sine factors of every distinct shape go up in one copy, one launch takes the signs. */
int cvh_init_checkerboard_batch(cvh_context *const *ctxs, int n);
int cvh_get_mask_device_batch(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, int invert, void *stream);

/* ---- Level-set reinitialisation --------------------------------------------------------------------------------------------
 * The reference's README lists it first under "Further ideas" ("add level set reinitialization ... avoids flattening of the
 * zero-level set"); it has no code for it.  cvh_reinit replaces the current level set u by the exact signed Euclidean distance to the
 * front of its own mask, on the device -- what a caller otherwise does with cvh_get_levelset, a CPU distance transform and
 * cvh_set_levelset.  The result is defined in integers:
 *   m(p)  = ((float)u(p) > 0), cvh_get_mask's rule (NaN, -0.0 and a positive double that rounds to 0.0f are outside);
 *   d2(p) = min over the pixels q with m(q) != m(p) of (p.row - q.row)^2 + (p.col - q.col)^2;
 *   u'(p) = m(p) ? sqrt((double)d2) - 0.5 : -(sqrt((double)d2) - 0.5), IEEE sqrt and one subtraction.
 * The zero level sits halfway between neighbouring pixels of opposite class (the front is quantised to pixel edges), |u'| >= 0.5
 * everywhere, and the mask is unchanged bit for bit.  A UNIFORM mask (no pixel of the other class) is not an error: the level set
 * and the context -- its run state included -- stay exactly as they are and *changed is 0.  Otherwise *changed is 1 and a new run
 * begins exactly as after cvh_set_levelset of the same values (with "state" = 32 the class is taken from the float state and the new
 * values are the doubles above rounded to float).  Iterations in flight are settled first.  `changed` may be NULL.
 * cvh_reinit_batch serves n contexts of one device, of any mix of shapes and channel counts, with ONE set of three launches on member
 * 0's stream, joined with every member's stream before and after as cvh_init_checkerboard_batch; changed is an array of n or NULL.
 * cvh_reinit is the same kernels with n = 1.  One host wait per call (which members changed).
 * How: a separable exact distance transform (chan_vese_amd/csrc/reinit_kernels.hip) -- a column pass in bands of 32 rows with a
 * fix-up across bands gives the vertical distances to both classes, a row pass minimises k^2 + g(j +- k)^2 outwards from LDS-held
 * rows and stops at k^2 >= best.  Its cost depends on the distances: per pixel the row pass makes at most min(vertical distance,
 * columns to the farther edge) trips.  Steady-state figures are not measured yet (tools/reinit_probe.py records us per call
 * beside the us of one CSV iteration of the same plane); host clocks around a context's FIRST call at 4096^2, allocation included:
 * 9.5 ms for the BASELINE disk's level set (distances in four digits), 1.4 ms for a noisy one -- upper bounds of about 150 and 20
 * CSV iterations of that plane (profiles/r09_reinit/).  The kernels move 24.25 bytes per pixel (read u 8, class words 0.25, distance
 * fields 4 + 4, write u' 8) against the floor of 16.
 * The workspace (4.125 bytes per pixel) is allocated by a context's first reinitialisation and kept; cvh_create allocates nothing
 * for it and the automatic choices that weigh the contexts of a device do not count it.
 * CVH_ERR_STATE: a member without a level set.  CVH_ERR_ARG: ctxs NULL, n < 1, a NULL or duplicate member, members on different
 * devices, a plane with h^2 + w^2 >= 2^32 (d2 is held in 32 bits).  Checked for every member before anything is launched; the message
 * names the member index and is cvh_last_error(NULL)'s and member 0's. */
int cvh_reinit(cvh_context *ctx, int *changed);
int cvh_reinit_batch(cvh_context *const *ctxs, int n, int *changed);

/* ---- Connected components of the mask ----------------------------------------------------------------------------------------
 * The reference says what its contour is for: "the resulting contour is used to cut out ROI".  On noisy images the mask has speckle,
 * pin-holes and several blobs; these calls label, measure and clean it ON THE DEVICE -- what a caller otherwise does with
 * cvh_get_mask, scipy.ndimage.label / cv::connectedComponents on a CPU and an upload.  They only read the level set: level set, run
 * state, sums and options are not touched, and a run continued after any of them is bit-identical to one without.  Iterations in flight
 * are settled first, as the getters do.  Everything is defined in integers:
 *   foreground  f(p) = (((float)u(p) > 0) != invert), cvh_get_mask's rule (NaN, -0.0 and a positive double that rounds to 0.0f are
 *               outside; with "state" = 32 the class comes from the float state, as in cvh_reinit);
 *   conn        4 or 8; the BACKGROUND uses the complementary connectivity (8 when conn = 4, 4 when conn = 8);
 *   labels      int32, row-major h x w, 0 = background; the foreground components are numbered 1..K in increasing order of their
 *               smallest flat index row*w + col -- scipy.ndimage.label's numbering (cross structure for 4, ones((3,3)) for 8);
 *   table       row k-1 describes label k: first = its smallest flat index, area, and the inclusive box x0 <= col <= x1, y0 <= row <= y1;
 *   cleaning    given min_area >= 0, fill_holes >= -1 and keep_largest in {0, 1}, in this order:
 *               1. foreground components with area < min_area are dropped;
 *               2. a hole is a background component of the result of 1, in the complementary connectivity, without a pixel in the
 *                  first or last row or column; every hole of area <= fill_holes becomes foreground (-1: holes of any size, 0: none);
 *               3. with keep_largest only the largest foreground component (conn) of the result of 2 stays; ties go to the smaller first.
 *               The output is a 0/1 uint8 mask; with (0, 0, 0) it is cvh_get_mask's, byte for byte (the existing mask kernel alone runs).
 * An all-background plane has K = 0, an all-zero label plane and an all-zero clean mask: no error.
 * cvh_components: d_labels (device, 4-byte aligned) may be NULL, table (host, cap rows) may be NULL, count may be NULL.  *count is always
 * the full K; table receives the first min(K, cap) rows.  cvh_components_batch: d_labels may be NULL and so may any of its entries (no
 * label plane for that member); counts is an array of n or NULL.
 * Device pointers follow the rules of "Device-memory input and output" above (hipPointerGetAttributes check, any byte alignment for
 * uint8, event ordering against `stream`).  The *_batch forms serve n contexts of one device, any mix of shapes and channel counts, with
 * ONE set of launches on member 0's stream, joined with every member's stream before and after as cvh_reinit_batch; the single-context
 * forms are the same kernels with n = 1.
 * Host waits: cvh_components and cvh_components_batch wait ONCE per call, for the counts; cvh_components waits a SECOND time where it
 * fills a table (K decides where the rows live; the rows are computed behind the first wait).  The clean-mask calls never need K on the
 * host: the device forms wait only where cvh_get_mask_device does, cvh_get_mask_clean once for its bytes as cvh_get_mask.
 * How (chan_vese_amd/csrc/components_kernels.hip): union-find with the smallest flat index as root, unions by atomic min on the larger
 * root, a lane per pixel; the launches are ordered by kernel boundaries alone.  A component's root is its `first` whatever the timing, so
 * labels, table and clean mask do not depend on the grid or the schedule.  Roots are numbered by per-workgroup counts and a
 * one-workgroup scan.  Cost: not measured (data flow, bytes per pixel, registers).
 * The workspace -- 8 bytes per pixel (parent / label words, per-root statistics) plus 4 bytes per 256 pixels (root counts), reused by
 * the second and third labelling of a clean mask; and 24 bytes per component for the rows of a table, where one is asked for -- is
 * allocated by a context's first call and kept until cvh_destroy; cvh_create allocates nothing for it and the automatic choices that
 * weigh the contexts of a device do not count it.
 * CVH_ERR_ARG: conn not 4 or 8, negative min_area, fill_holes < -1, keep_largest not 0 or 1, negative cap, ctxs NULL, n < 1, a NULL or
 * duplicate member, members on different devices, a NULL mask pointer, a pointer that is not device-accessible memory of the
 * context's device or a misaligned label plane, a plane with h*w >= 2^31.  CVH_ERR_STATE: a member without a level set.  Checked for
 * every member before anything is launched; the message names the member index and is cvh_last_error(NULL)'s and member 0's. */
typedef struct cvh_component { uint32_t first, area; int32_t x0, y0, x1, y1; } cvh_component;

int cvh_components(cvh_context *ctx, int conn, int invert, int32_t *d_labels, cvh_component *table, int cap, int *count, void *stream);
int cvh_components_batch(cvh_context *const *ctxs, int n, int conn, int invert, int32_t *const *d_labels, int *counts, void *stream);
int cvh_get_mask_clean(cvh_context *ctx, uint8_t *mask, int conn, int invert, long min_area, long fill_holes, int keep_largest);
int cvh_get_mask_clean_device(cvh_context *ctx, uint8_t *d_mask, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                              void *stream);
int cvh_get_mask_clean_device_batch(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, int conn, int invert, long min_area,
                                    long fill_holes, int keep_largest, void *stream);

/* ---- Device-side initial level sets -------------------------------------------------------------------------------------------
 * The reference's "greater picture" wants its input parameters "found by analyzing the original image".  Chan-Vese minimises the
 * within-region variance and Otsu's threshold minimises the same quantity over thresholds of the grey values, so an Otsu start is
 * already close to the answer.  These calls build a start ON THE DEVICE -- what a caller otherwise fills on the host and uploads at
 * 8 bytes per pixel with cvh_set_levelset.  Everything is defined in integers:
 *   grey value  g(p) = sum_k I_k(p) over the context's C planes as they are now (after cvh_perona_malik: the smoothed planes), 0 .. 255 C;
 *   histogram   B = 255 C + 1 bins (256 or 766), hist[v] = the number of pixels with g = v;
 *   Otsu t      with N = h w, S = sum v hist[v], n0(t) = sum_{v<=t} hist[v], s0(t) = sum_{v<=t} v hist[v]: the candidates are the t in
 *               0 .. B-2 with 0 < n0(t) < N; a candidate's score is ((double)d * (double)d) / (double)q with d = S n0 - N s0 (an exact
 *               integer: 128 bits) and q = n0 (N - n0) (exact), each conversion rounded to nearest even, one IEEE multiply and one IEEE
 *               divide -- Python's float(d) * float(d) / float(q) on integers; t is the candidate with the largest score, ties to the
 *               smallest t.  A plane with a single occupied bin v0 has no candidate: t = v0, no error (its threshold start is uniformly
 *               outside);
 *   threshold   u(p) = g(p) > t ? inside : outside;
 *   rect        (x, y, rw, rh), rw > 0, rh > 0: inside where x <= col < x + rw and y <= row < y + rh, clipped to the plane, else outside;
 *               an empty intersection gives a uniform plane, no error;
 *   disk        (cx, cy, r), r >= 0: inside where (col - cx)^2 + (row - cy)^2 <= r^2 in 64-bit integers -- a FILLED disk (the CLI's
 *               --circ, the reference's 1-pixel outline, is something else and stays on the host).
 * inside and outside are any doubles, NaN included, stored bit for bit.  Each start leaves the context exactly as cvh_set_levelset of
 * the same doubles would: a new run begins (counter, stop flag, sums; with "state" = 32 the float pair adopts the level set), done as
 * cvh_init_checkerboard_batch does it.  Iterations in flight are settled first.  cvh_histogram*, cvh_otsu_threshold only READ the planes:
 * level set, run state, sums and options are not touched, and a run continued after them is bit-identical to one without.
 * cvh_histogram: hist is a HOST buffer of cap counters (may be NULL when cap is 0); the first min(B, cap) bins are copied, *bins (may be
 * NULL) is always B.  cvh_histogram_batch: hists and caps are arrays of n.  cvh_otsu_from_histogram is a host-only helper (1 <= bins <=
 * 766, CVH_ERR_ARG for an empty histogram), like cvh_levelset_checkerboard_host.  cvh_init_otsu[_batch]: t (one int / an array of n)
 * receives the thresholds and may be NULL.  xywh holds 4 n ints, cxcyr 3 n.
 * The *_batch forms serve n contexts of one device, any mix of shapes and channel counts, with ONE launch per kernel on member 0's
 * stream, joined with every member's stream before and after as cvh_init_checkerboard_batch; the single-context forms are the same
 * kernels with n = 1.  Host waits: one per call; cvh_init_otsu* two -- the histogram launch, a wait (the maximisation over at most 765
 * candidates runs on the host), the start launch, the closing wait.
 * How (chan_vese_amd/csrc/init_kernels.hip): the histogram kernel reads 16-byte pieces of the planes (1 byte per pixel and plane),
 * counts in LDS with equal values aggregated within a wave first -- a flat image sends every lane to one bin -- and flushes once per
 * workgroup with 32-bit atomics; the start kernel writes 16-byte pieces of the level set (8 bytes per pixel; the threshold start also
 * reads the planes).  Cost: not measured.  The histogram workspace (4 B bytes) is allocated by a context's first call
 * that needs it and kept until cvh_destroy.
 * CVH_ERR_ARG: NULL pointers, n < 1, a NULL or duplicate member, members on different devices, negative cap, t outside 0 .. B-1, rw or
 * rh <= 0, r < 0, a plane with h*w >= 2^32 (32-bit counters).  CVH_ERR_STATE: the histogram, Otsu and threshold calls on a member
 * without an image (rect and disk need none).  Checked for every member before anything is launched; the message names the member index
 * and is cvh_last_error(NULL)'s and member 0's.  CVH_ERR_HIP: a HIP call failed, or the histogram launch of an Otsu call came back
 * without a single counted pixel (nothing is started then). */
int cvh_histogram(cvh_context *ctx, uint32_t *hist, int cap, int *bins);
int cvh_histogram_batch(cvh_context *const *ctxs, int n, uint32_t *const *hists, const int *caps);
int cvh_otsu_from_histogram(const uint32_t *hist, int bins, int *t);
int cvh_otsu_threshold(cvh_context *ctx, int *t);
int cvh_init_threshold(cvh_context *ctx, int t, double inside, double outside);
int cvh_init_threshold_batch(cvh_context *const *ctxs, int n, const int *t, double inside, double outside);
int cvh_init_otsu(cvh_context *ctx, int *t, double inside, double outside);
int cvh_init_otsu_batch(cvh_context *const *ctxs, int n, int *t, double inside, double outside);
int cvh_init_rect(cvh_context *ctx, int x, int y, int rw, int rh, double inside, double outside);
int cvh_init_rect_batch(cvh_context *const *ctxs, int n, const int *xywh, double inside, double outside);
int cvh_init_disk(cvh_context *ctx, int cx, int cy, int r, double inside, double outside);
int cvh_init_disk_batch(cvh_context *const *ctxs, int n, const int *cxcyr, double inside, double outside);

/* ---- Coarse-to-fine ---------------------------------------------------------------------------------------------------------
 * A plane that fits the LDS of the chip iterates several times cheaper per iteration than a large one (README), so a pyramid does most
 * of its iterations on small planes and only the last few on the full plane.  These calls move the planes DOWN and the level set UP
 * between two contexts of one device with the same channel count, the coarse one exactly ((h + 1) / 2) x ((w + 1) / 2) for a fine
 * h x w (integer division) -- what a caller otherwise does with cvh_get_image, a CPU average and cvh_set_image, and with
 * cvh_get_levelset, a CPU replication and cvh_set_levelset at 8 bytes per pixel.  Both are defined in integers or as bit copies:
 *   restrict  per plane k of the fine context as it is now (after cvh_perona_malik: the smoothed plane), for coarse pixel (r, c) with
 *             r0 = 2r, r1 = min(2r + 1, h - 1), c0 = 2c, c1 = min(2c + 1, w - 1):
 *               coarse_k(r, c) = (f(r0, c0) + f(r0, c1) + f(r1, c0) + f(r1, c1) + 2) >> 2
 *             (an odd last row or column counts its pixels twice).  The coarse context is left exactly as cvh_set_image of those bytes
 *             leaves it -- planes, sums, stop norm, validity flags; its level set, if any, stays as cvh_set_image leaves it.  The fine
 *             context is only read: level set, run state, sums and options are untouched (iterations it has in flight stay in flight),
 *             and a run continued after the call is bit-identical to one without.
 *   prolong   u_fine(r, c) = u_coarse(r >> 1, c >> 1), BIT FOR BIT -- NaN payloads, -0.0, infinities and denormals included; no scaling,
 *             no interpolation: the sign pattern, and so the mask, is replicated exactly.  The source values are those cvh_get_levelset
 *             of the coarse context returns (with "state" = 32 the exact doubles of its floats); its iterations in flight are settled
 *             first, as the getters do, and it is only read.  The fine context is left exactly as cvh_set_levelset of those doubles
 *             leaves it: a new run begins, and with "state" = 32 its float pair adopts the level set (as cvh_init_*).
 * The *_batch forms take n pairs (pair i = fines[i], coarses[i]) of any mix of shapes and channel counts in ONE launch on the stream of
 * pair 0's DESTINATION (restrict: coarses[0]; prolong: fines[0]), ordered after everything already enqueued on the streams of both
 * contexts of every pair and before anything enqueued on them later; one host wait per call (restrict: the sums come back -- one
 * channel summed on the device, three channels fetched and summed on the host behind that wait, as cvh_set_image_device_batch).  The
 * single-pair forms are the same kernels with n = 1.
 * A pyramid is then: restrict down the chain; build the start on the coarsest level (any cvh_init_*: a threshold or Otsu start acts on
 * the coarsest planes); run the coarsest level; prolong; run the next level; ... -- every level with its own parameters and options,
 * nothing is rescaled (the level set's magnitudes carry over; mu, eps and tol mean on every level what they mean on a lone context).
 * For the automatic choices see "co_resident" above.  capi.run_coarse_to_fine, Segmenter(levels=) and chan_vese --levels do this.
 * How (chan_vese_amd/csrc/pyramid_kernels.hip): pure streaming over the member table.  Restrict: a lane makes 16 coarse pixels from two
 * 32-byte runs of fine bytes (16-byte loads, one 16-byte store), 5 bytes per coarse pixel and plane.  Prolong: a lane reads a 16-byte
 * piece of a coarse row and writes each value twice into two fine rows (16-byte stores), 40 bytes per coarse pixel.  Cost, one run
 * of tools/pyramid_probe.py on an MI355X: a call with its wait 54 / 59 us at 4096^2 -> 2048^2 -- about one CSV
 * iteration of the 4096^2 plane; a noisy 4096^2 disk from the checkerboard 44.6 ms of CSV device time in one level, 9.3 ms in three.
 * CVH_ERR_ARG: NULL lists or members, n < 1, a context listed more than once across both lists (fine == coarse included), contexts on
 * different devices within or across pairs, different channel counts within a pair, a coarse shape other than the one above, a fine
 * plane with h*w >= 2^32.  CVH_ERR_STATE: restrict from a context without an image, prolong from one without a level set.  Checked for
 * every pair before anything is launched; the message names the pair index and is cvh_last_error(NULL)'s (and pair 0's destination's,
 * once the lists hold no NULL); the contexts stay usable. */
int cvh_restrict_image(cvh_context *fine, cvh_context *coarse);
int cvh_restrict_image_batch(cvh_context *const *fines, cvh_context *const *coarses, int n);
int cvh_prolong_levelset(cvh_context *coarse, cvh_context *fine);
int cvh_prolong_levelset_batch(cvh_context *const *coarses, cvh_context *const *fines, int n);

/* ---- Colour spaces ----------------------------------------------------------------------------------------------------------
 * In RGB every plane is "brightness plus a bit of hue", so the per-channel lambda1[k] / lambda2[k] buy little.  Split into a luma plane
 * and two chroma planes, the same three weights say "ignore shading, follow hue" (lambda = 0, 1, 1).  These calls convert the three
 * planes of a context in place on the device, and write the luma of a three-channel context into a one-channel context -- what a
 * caller otherwise does with cvh_get_image, a host conversion and cvh_set_image at 6 bytes per pixel across PCIe.  The reference has
 * no code for this; the definition below IS the contract.  Its constants are those of OpenCV's 8-bit cvtColor, but parity with OpenCV
 * is not pinned by any test.
 *   order  says which plane of the context is which primary: CVH_ORDER_BGR plane 0 = B, 1 = G, 2 = R (cv::split of cv::imread; the
 *          CLI); CVH_ORDER_RGB plane 0 = R, 1 = G, 2 = B.
 *   space  CVH_COLOUR_YCRCB or CVH_COLOUR_YUV.
 * All arithmetic is in signed 32-bit integers; >> is the arithmetic shift (floor); sat(x) = min(max(x, 0), 255); H = 8192;
 * D = 128 << 14.  Forward, per pixel:
 *     Y = (4899 R + 9617 G + 1868 B + H) >> 14          (the weights add up to 2^14: 0 <= Y <= 255 without a clamp)
 *     YCrCb  plane 0 = Y, plane 1 = Cr = sat(((R - Y) * 11682 + D + H) >> 14), plane 2 = Cb = sat(((B - Y) *  9241 + D + H) >> 14)
 *     YUV    plane 0 = Y, plane 1 = U  = sat(((B - Y) *  8061 + D + H) >> 14), plane 2 = V  = sat(((R - Y) * 14369 + D + H) >> 14)
 * The output planes are always (Y, second, third), whatever `order` was: lambda1[0] / lambda2[0] weigh the luma.  Inverse, planes
 * (Y, P1, P2) read and R, G, B written back in `order`, with a(x) = x - 128:
 *     YCrCb  R = sat(Y + ((a(Cr) * 22987 + H) >> 14)), G = sat(Y + ((a(Cb) * -5636 + a(Cr) * -11698 + H) >> 14)),
 *            B = sat(Y + ((a(Cb) * 29049 + H) >> 14))
 *     YUV    R = sat(Y + ((a(V) * 18678 + H) >> 14)),  G = sat(Y + ((a(U) * -6472 + a(V) * -9519 + H) >> 14)),
 *            B = sat(Y + ((a(U) * 33292 + H) >> 14))
 * Facts of this definition over all 2^24 colours (tests/test_colour_api.py): Y spans 0 .. 255; the raw Cr (before sat) spans 0 .. 256
 * -- one value clamps --, the raw Cb 1 .. 255; the raw V spans -29 .. 285 -- it clamps --, the raw U 17 .. 239; a grey pixel
 * (R = G = B = v) maps to (v, 128, 128) and back to itself exactly, in both spaces; the round trip changes each of R, G, B by at most 1
 * for YCrCb; for YUV it changes R by up to 34 and G by up to 17, where V clamped, and B by at most 1.
 *   cvh_convert_colour*  replaces the three planes of every member in place (inverse = 0 forward, 1 back).  The source is the planes as
 *             they are now (after cvh_perona_malik: the smoothed planes).  Every member is left exactly as cvh_set_image of the
 *             converted bytes leaves it -- planes, sums, stop norm, validity flags; a level set it already has stays as cvh_set_image
 *             leaves it; iterations in flight are settled first, as cvh_set_image does.  The library keeps NO record of the space a
 *             context's planes are in: planes are bytes, and converting twice or inverting what was never converted is the caller's
 *             business, well defined by the formulas.
 *   cvh_luma_image*      writes the Y of src (three channels) into the single plane of dst, a one-channel context of the same h x w on
 *             the same device, which is left exactly as cvh_set_image of that plane leaves it (its sums taken on the device in the
 *             same launch, exact integers).  src is only read: level set, run state, sums and options are untouched, its iterations in
 *             flight stay in flight, and a run continued after the call is bit-identical to one without (as cvh_restrict_image).
 * The *_batch forms take n members or pairs (pair i = srcs[i], dsts[i]) of any mix of shapes in ONE launch -- convert on member 0's
 * stream, luma on the stream of pair 0's destination --, ordered after everything already enqueued on the stream of every listed
 * context and before anything enqueued on them later; one host wait per call, for the sums (one channel summed on the device, three
 * channels fetched and summed on the host behind that wait, as cvh_set_image_device_batch).  The single forms are the same kernels
 * with n = 1.
 * How (chan_vese_amd/csrc/colour_kernels.hip): pure streaming over the member table; a lane takes a 16-byte piece (16 pixels) of each
 * plane, computes from byte-extracted words and stores three pieces in place (6 bytes per pixel) or one (luma: 4 bytes per pixel).
 * Cost, one run of tools/colour_probe.py on an MI355X (host clock around a call and its wait, 20 calls): luma 47 / 60 /
 * 75 us at 1024^2 / 2048^2 / 4096^2 -- about one CSV iteration of the 4096^2 x 3 plane (82 us); convert 1.2 / 4.6 / 13.1 ms, nearly
 * all of it the three-channel stop norm the host takes behind the wait, as for every call that replaces three planes.
 * CVH_ERR_ARG: NULL lists or members, n < 1, a context listed more than once (across both lists for luma, src == dst included),
 * contexts on different devices, an unknown space or order, inverse other than 0 or 1, a member of convert or a src of luma that has
 * not 3 channels, a dst that has not 1 channel or has another shape, h*w >= 2^32.  CVH_ERR_STATE: a member or src without an image.
 * Checked for every member or pair before anything is launched; the message names its index and is cvh_last_error(NULL)'s (and the
 * leader's, once the lists hold no NULL); the contexts stay usable and their planes unchanged. */
#define CVH_ORDER_BGR 0
#define CVH_ORDER_RGB 1
#define CVH_COLOUR_YCRCB 1
#define CVH_COLOUR_YUV 2
int cvh_convert_colour(cvh_context *ctx, int space, int order, int inverse);
int cvh_convert_colour_batch(cvh_context *const *ctxs, int n, int space, int order, int inverse);
int cvh_luma_image(cvh_context *src, cvh_context *dst, int order);
int cvh_luma_image_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, int order);

/* ---- Local statistics ---------------------------------------------------------------------------------------------------------
 * The model separates regions by their per-channel means, so two regions of the same mean and different texture look alike to it.
 * A plane of the local standard deviation tells them apart, and it is a uint8 plane like any other: the iteration kernels run on it
 * unchanged, and lambda1[k] / lambda2[k] say how much each of brightness and texture counts.  These calls write such planes on the
 * device -- what a caller otherwise does with cvh_get_image, a host filter and cvh_set_image.  The reference has no code for this;
 * the definition below IS the contract.
 *   Pairs.  src and dst are different contexts of the same h x w on the same device; each has 1 or 3 channels, independently.  Plane
 *          k of dst becomes f_what[k] of plane min(k, C_src - 1) of src, taken as the planes are now (after cvh_perona_malik: the
 *          smoothed planes).  Entries of `what` at k >= C_dst are ignored.  A grey src and a three-channel dst with what = (COPY,
 *          MEAN, DEV) is the texture stack; 3 -> 3 with (DEV, DEV, DEV) is per-channel texture; 1 -> 1 with DEV the texture plane alone.
 *   Definition.  All arithmetic is unsigned 64-bit and / is floor division.  For pixel (r, c) and radius R the window is rows
 *          max(r - R, 0) .. min(r + R, h - 1) and columns max(c - R, 0) .. min(c + R, w - 1): truncated at the border, nothing is
 *          padded.  With n the window's pixel count, S = sum p and Q = sum p^2 over the window:
 *              CVH_LOCAL_COPY   p
 *              CVH_LOCAL_MEAN   (2 S + n) / (2 n)                     round-half-up; never above 255
 *              CVH_LOCAL_DEV    isqrt(4 (n Q - S^2) / n^2)            isqrt: the exact floor square root
 *          DEV is floor(2 sigma) of the window's population deviation; 4 sigma^2 <= 255^2 = 65025, so DEV <= 255 without a clamp.
 *          With R <= CVH_LOCAL_RADIUS_MAX: n <= 65025 and 4 n Q < 2^51.  R = 0 gives MEAN = p and DEV = 0; a constant plane gives MEAN = the constant and DEV = 0; a window half a and half b gives DEV = |a - b|.
 *   State. dst is left exactly as cvh_set_image of those bytes leaves it -- planes, sums, stop norm, validity flags; a level set it
 *          already has stays as cvh_set_image leaves it; its iterations in flight are settled first.  src is only read: level set,
 *          run state, sums and options are untouched, its iterations in flight stay in flight, and a run continued after the call is
 *          bit-identical to one without (as cvh_luma_image).
 * The *_batch form takes n pairs (pair i = srcs[i], dsts[i], radius[i], what[CVH_MAX_CHANNELS * i ..]) of any mix of shapes, channel
 * counts, radii and codes in ONE set of launches on the stream of pair 0's destination, ordered after everything already enqueued on
 * the stream of every listed context and before anything enqueued on them later; one host wait per call, for the sums (one channel
 * summed on the device, three channels fetched and summed on the host behind that wait, as cvh_luma_image_batch).  The single form is
 * the batch with n = 1; a member alone or in any batch gets the same bytes.
 * How (chan_vese_amd/csrc/local_kernels.hip): the window sums are separable, so the work per pixel does not grow with R^2.  A row
 * pass writes the horizontal window sums of every source plane a MEAN or DEV plane reads -- prefix sums of a row segment in LDS, a
 * pixel's sum the difference of two entries -- into a workspace the destination owns (6 bytes per pixel and plane, allocated by its
 * first such call, freed by cvh_destroy).  In the column pass a wave takes a band of 32 rows by 256 columns, each lane holding the
 * running vertical sums of four columns in registers; it reads the 2 R + 1 rows about the band's first row, then adds one row and
 * subtracts one per row written.  A call of COPY planes alone skips the row pass.
 * Cost, one run of tools/local_probe.py on an MI355X (profiles/r19_local/; host clock around a call and its wait, 20
 * calls after 3): the 1 -> 1 deviation plane at R = 2 / 8 / 32 / 127 takes 115 / 120 / 134 / 198 us at 1024^2, 128 / 134 / 153 / 209 us
 * at 2048^2 and 181 / 186 / 201 / 281 us at 4096^2 -- NOT flat in R: the row pass does not depend on R, but a band of 32 rows starts
 * from 2 R + 1 rows of row sums (69 row reads per band at R = 2, 319 at R = 127), and the call is 55 - 70 % dearer at R = 127 than at
 * R = 2.  One CSV iteration of the same plane: 10 / 14 / 65 us.  The 1 -> 3 stack takes 1.1 / 4.0 / 12.9 ms at every radius, nearly
 * all of it the three-channel stop norm the host takes behind the wait, as for every call that replaces three planes.  The round trip
 * the call replaces (cvh_get_image, numpy cumulative sums, cvh_set_image) took 56 ms / 0.39 s / 3.2 s in the same run.
 * CVH_ERR_ARG: NULL lists or members, n < 1, a context listed more than once across both lists (src == dst included), contexts on
 * different devices, different shapes within a pair, a radius outside 0 .. CVH_LOCAL_RADIUS_MAX, a `what` entry below C_dst that is
 * none of the three codes, h*w >= 2^32.  CVH_ERR_STATE: a src without an image.  Checked for every pair before anything is launched;
 * the message names the pair index and is cvh_last_error(NULL)'s (and pair 0's destination's, once the lists hold no NULL); the
 * contexts stay usable and their planes unchanged. */
#define CVH_LOCAL_COPY 0
#define CVH_LOCAL_MEAN 1
#define CVH_LOCAL_DEV  2
#define CVH_LOCAL_RADIUS_MAX 127
int cvh_local_planes(cvh_context *src, cvh_context *dst, int radius, const int *what);
int cvh_local_planes_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n,
                           const int *radius /* n */, const int *what /* CVH_MAX_CHANNELS per pair */);

/* ---- Rank planes --------------------------------------------------------------------------------------------------------------
 * Two failures of a model that separates regions by their global means have classical answers in rank filters.  Impulse noise: an
 * isolated 0 or 255 pixel survives Perona-Malik as an edge; a median removes it.  Uneven illumination of a grey image: the run
 * segments the shading ramp, not the objects; the white top-hat -- the image minus its grey opening by a window wider than the
 * objects -- removes the ramp.  These calls write such planes on the device -- what a caller otherwise does with cvh_get_image, a
 * host filter and cvh_set_image.  The reference has no code for this; the definition below IS the contract.
 *   Pairs.  Exactly as "Local statistics": src and dst are different contexts of the same h x w on the same device; each has 1 or 3
 *          channels, independently.  Plane k of dst becomes f_what[k] of plane min(k, C_src - 1) of src, taken as the planes are now.
 *          Entries of `what` at k >= C_dst are ignored.
 *   Definition.  For pixel (r, c) and radius R the window is rows max(r - R, 0) .. min(r + R, h - 1) and columns max(c - R, 0) ..
 *          min(c + R, w - 1): truncated at the border, nothing is padded.  With n the window's pixel count and s[0] <= .. <= s[n-1]
 *          its bytes sorted:
 *              CVH_RANK_COPY    p
 *              CVH_RANK_MIN     s[0]
 *              CVH_RANK_MAX     s[n-1]
 *              CVH_RANK_MEDIAN  s[(n-1)/2]                            the lower median under floor division
 *              CVH_RANK_OPEN    MAX_R(MIN_R(p))                       both windows truncated as above
 *              CVH_RANK_CLOSE   MIN_R(MAX_R(p))
 *              CVH_RANK_TOPHAT  p - OPEN
 *              CVH_RANK_BOTHAT  CLOSE - p
 *          Truncated MIN and MAX are an adjoint erosion and dilation on the plane's own domain, so OPEN <= p <= CLOSE at every
 *          pixel, and TOPHAT and BOTHAT need no clamp.  R = 0 gives p for the first six codes and 0 for the two hats; a constant
 *          plane gives the constant and 0.  n <= 225 at R <= CVH_RANK_MEDIAN_RADIUS_MAX, so a count of window samples fits a byte:
 *          that is why the median's limit is 7.  The window is a square; there is no disk-shaped grey structuring element.
 *   State. As "Local statistics", word for word: dst is left exactly as cvh_set_image of those bytes leaves it -- planes, sums, stop
 *          norm, validity flags; a level set it already has stays as cvh_set_image leaves it; its iterations in flight are settled
 *          first.  src is only read: level set, run state, sums and options are untouched, its iterations in flight stay in flight,
 *          and a run continued after the call is bit-identical to one without.
 * The *_batch form takes n pairs (pair i = srcs[i], dsts[i], radius[i], what[CVH_MAX_CHANNELS * i ..]) of any mix of shapes, channel
 * counts, radii and codes in ONE set of launches on the stream of pair 0's destination, ordered after everything already enqueued on
 * the stream of every listed context and before anything enqueued on them later; one host wait per call, for the sums (one channel
 * summed on the device, three channels fetched and summed on the host behind that wait).  The single form is the batch with n = 1; a
 * member alone or in any batch gets the same bytes.
 * How (chan_vese_amd/csrc/rank_kernels.hip): MIN and MAX are separable, a row pass then a column pass, each by van Herk / Gil-Werman
 * (running extrema from both ends of blocks of 2 R + 1), so the work per pixel does not grow with R; OPEN and CLOSE are four passes,
 * the hats subtract in the last one; a plane that several codes of one member derive from is eroded and dilated once.  The median for
 * R = 1 .. 7 keeps a histogram of 256 byte counters per lane in LDS while the lane marches down a column: work per pixel O(R).
 * Between the passes the planes live at one byte per pixel in a workspace the destination owns (7 byte planes per plane of the
 * destination, allocated by its first call that takes anything but copies, freed by cvh_destroy); it shares no storage with the
 * workspace of "Local statistics".  A call of COPY planes alone launches only the writer.
 * Cost, MEASURED ONCE: one run of tools/rank_probe.py on an MI355X (profiles/r20_rank/; host clock around a call and
 * its wait, 20 calls after 3), 1 -> 1 at 1024^2 / 2048^2 / 4096^2: MAX at R = 2 takes 98 / 107 / 190 us and at R = 127 377 / 394 /
 * 511 us, TOPHAT 136 / 163 / 327 us and 680 / 719 / 939 us -- NOT flat in R: the work per pixel is, but a column band is 255 rows tall
 * at R = 127 and the column passes run out of parallel waves.  MEDIAN grows about linearly with R: 112 / 126 / 345 us at R = 1, 215 /
 * 243 / 869 us at R = 7.  One CSV iteration of the same plane: 8 / 14 / 67 us.  The round trip each call replaces (cvh_get_image, a
 * scipy filter, cvh_set_image) took 12 ms - 30 s in the same run: every call measured beats it.  A three-channel destination adds the
 * stop norm the host takes behind the wait (1 - 14 ms), as for every call that replaces three planes.  Device times of the kernels
 * alone were not taken.
 * CVH_ERR_ARG: everything cvh_local_planes_batch refuses, with the radius bound 0 .. CVH_RANK_RADIUS_MAX -- NULL lists or members,
 * n < 1, a context listed more than once across both lists (src == dst included), contexts on different devices, different shapes
 * within a pair, h*w >= 2^32 --; a `what` entry below C_dst outside 0 .. 7; a pair with a MEDIAN entry below C_dst and a radius above
 * CVH_RANK_MEDIAN_RADIUS_MAX.  CVH_ERR_STATE: a src without an image.  Checked for every pair before anything is launched; the message
 * names the pair index and is cvh_last_error(NULL)'s (and pair 0's destination's, once the lists hold no NULL); the contexts stay
 * usable and their planes unchanged. */
#define CVH_RANK_COPY   0
#define CVH_RANK_MIN    1
#define CVH_RANK_MAX    2
#define CVH_RANK_MEDIAN 3
#define CVH_RANK_OPEN   4
#define CVH_RANK_CLOSE  5
#define CVH_RANK_TOPHAT 6
#define CVH_RANK_BOTHAT 7
#define CVH_RANK_RADIUS_MAX        127
#define CVH_RANK_MEDIAN_RADIUS_MAX 7
int cvh_rank_planes(cvh_context *src, cvh_context *dst, int radius, const int *what);
int cvh_rank_planes_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n,
                          const int *radius /* n */, const int *what /* CVH_MAX_CHANNELS per pair */);

/* ---- Smoothing ----------------------------------------------------------------------------------------------------------------
 * A weighted window: the Gaussian blur that the two sections above do not have, and any other symmetric separable kernel.  Its uses
 * here: the textbook edge function of "Edge-weighted length", g = 1 / (1 + |grad (G_sigma * I)|^2 / K^2), built from a blurred copy
 * while the run keeps the unsmoothed planes; and p minus its smooth background, the flat-field step of microscopy.  These calls
 * write such planes on the device -- what a caller otherwise does with cvh_get_image, a host filter and cvh_set_image.  The
 * reference has no code for this; the definition below IS the contract, in integers, so every byte is defined.
 *   Pairs.  Exactly as "Local statistics": src and dst are different contexts of the same h x w on the same device; each has 1 or 3
 *          channels, independently.  Plane k of dst becomes f_what[k] of plane min(k, C_src - 1) of src, taken as the planes are now.
 *          Entries of `what` at k >= C_dst are ignored.
 *   Taps.  A pair has a radius R, 0 <= R <= CVH_SMOOTH_RADIUS_MAX, and R + 1 taps t[0 .. R] of 15-bit fixed point; the kernel is
 *          symmetric, t[-i] = t[i], and t[0] + 2 sum_{i >= 1} t[i] must be exactly 32768.  Nothing else is asked: a box or a
 *          binomial is as legal as a Gaussian, and the taps need not decay.
 *   Border. Indices are CLAMPED to the plane (replicate; scipy's mode='nearest') -- NOT the truncated window of the two sections
 *          above: a weight sum that changes per pixel would cost a division per pixel and pass.
 *   Definition.  All sums are exact integers and >> is the arithmetic shift; each rounding is shown once.
 *              row pass     a(x, y) = sum_{i = -R .. R} t[|i|] p(clamp(x + i, 0, w - 1), y)             below 2^23
 *                           v = (a + 64) >> 7                    8.8 fixed point, at most 65280: a uint16_t
 *              column pass  b(x, y) = sum_{j = -R .. R} t[|j|] v(x, clamp(y + j, 0, h - 1))             at most 65280 * 32768 < 2^31
 *                           BLUR = (b + 2^22) >> 23              0 .. 255
 *              CVH_SMOOTH_COPY    p
 *              CVH_SMOOTH_BLUR    as above
 *              CVH_SMOOTH_DETAIL  min(255, max(0, 128 + p - BLUR))
 *          A constant plane c gives BLUR = c and DETAIL = 128; R = 0 (t[0] = 32768) gives BLUR = p.
 *   State. As "Local statistics", word for word: dst is left exactly as cvh_set_image of those bytes leaves it; src is only read.
 * cvh_gauss_taps(sigma, taps, radius) is the definition of THE Gaussian of this library (host only, no context; the Python binding
 * and the command line call it and never restate it): sigma finite, 0 < sigma <= 21; *radius = R = ceil(3 sigma); in double,
 * e_i = exp(-i^2 / (2 sigma^2)) and S = e_0 + 2 sum_{i >= 1} e_i; taps[i] = floor(32768 e_i / S + 0.5) for i = 1 .. R and taps[0] =
 * 32768 - 2 sum_{i >= 1} taps[i].  `taps` has room for CVH_SMOOTH_RADIUS_MAX + 1 entries; those behind R are set to 0.  The centre
 * tap absorbs the rounding residue, so it need not be the largest: at sigma = 21 it is 618 below taps[1] = 623.  That is expected,
 * and legal.  CVH_ERR_ARG (message in cvh_last_error(NULL)): a sigma outside that range or not finite, a NULL pointer.
 * The *_batch form takes n pairs (pair i = srcs[i], dsts[i], radius[i], taps[i][0 .. radius[i]], what[CVH_MAX_CHANNELS * i ..]) of any
 * mix of shapes, channel counts, radii, taps and codes in ONE set of launches on the stream of pair 0's destination, ordered and
 * waited for as cvh_local_planes_batch.  The single form is the batch with n = 1; a member alone or in any batch gets the same bytes.
 * How (chan_vese_amd/csrc/smooth_kernels.hip; the two roundings: smooth_math.h): the pairs' taps go up beside the member table, 128
 * bytes per pair.  The row pass stages a row segment of 1024 columns and R columns on either side in LDS, clamped, and a lane adds
 * up t[i] (p[x - i] + p[x + i]) for its columns; v goes as 16 bits into a workspace the destination owns (2 bytes per pixel and
 * plane of the destination, allocated by its first call that takes anything but copies, freed by cvh_destroy; it shares no storage
 * with the workspaces of the two sections above).  In the column pass a workgroup holds 256 rows of v by 64 columns in LDS (32 KiB):
 * the 256 - 2 R rows of its band and R rows on either side, clamped; a lane owns a column.  The work per pixel grows linearly with R,
 * as the median's does; larger scales are what cvh_restrict_image is for.  A call of COPY planes alone launches only the writer and
 * allocates nothing.
 * Cost, MEASURED ONCE: one run of tools/smooth_probe.py on an MI355X (profiles/smooth/; host clock around a call and
 * its wait, 20 calls after 3), BLUR 1 -> 1 at sigma = 1 / 3 / 10 / 21 (R = 3 / 9 / 30 / 63): 84 / 91 / 116 / 134 us at 1024^2, 93 / 103 /
 * 145 / 184 us at 2048^2, 138 / 176 / 282 / 466 us at 4096^2 -- it grows with R, as said.  cvh_local_planes MEAN at the same R in the
 * same run: 92 / 97 / 111 / 131, 106 / 111 / 126 / 146 and 151 / 157 / 174 / 203 us: the blur is the cheaper call up to R = 9 and LOSES
 * from R = 30 on, by 2.3 x at 4096^2 and R = 63.  One CSV iteration of the same plane: 7 / 14 / 67 us.  The round trip the call replaces
 * (cvh_get_image, scipy's gaussian_filter, cvh_set_image) took 10 - 45 ms, 37 - 188 ms and 0.22 - 0.89 s.
 * CVH_ERR_ARG: everything cvh_local_planes_batch refuses, with the radius bound 0 .. CVH_SMOOTH_RADIUS_MAX -- NULL lists or members,
 * n < 1, a context listed more than once across both lists (src == dst included), contexts on different devices, different shapes
 * within a pair, h*w >= 2^32 --; a `what` entry below C_dst outside 0 .. 2; a NULL list of taps or a NULL entry of it; taps whose
 * t[0] + 2 sum t[i] is not 32768.  CVH_ERR_STATE: a src without an image.  Checked for every pair before anything is launched; the
 * message names the pair index and is cvh_last_error(NULL)'s (and pair 0's destination's, once the lists hold no NULL); the contexts
 * stay usable and their planes unchanged. */
#define CVH_SMOOTH_COPY   0
#define CVH_SMOOTH_BLUR   1
#define CVH_SMOOTH_DETAIL 2
#define CVH_SMOOTH_RADIUS_MAX 63
#define CVH_SMOOTH_TAP_SUM 32768
int cvh_gauss_taps(double sigma, uint16_t *taps /* CVH_SMOOTH_RADIUS_MAX + 1 */, int *radius);
int cvh_smooth_planes(cvh_context *src, cvh_context *dst, int radius, const uint16_t *taps, const int *what);
int cvh_smooth_planes_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n,
                            const int *radius /* n */, const uint16_t *const *taps /* n lists of radius[i] + 1 */,
                            const int *what /* CVH_MAX_CHANNELS per pair */);

/* ---- Energy ------------------------------------------------------------------------------------------------------------------
 * The library minimises the Chan-Sandberg-Vese functional
 *     E(u) = mu Length + nu Area + (1/C) sum_k [ lambda1_k int (I_k - c1_k)^2 H_eps(u) + lambda2_k int (I_k - c2_k)^2 (1 - H_eps(u)) ];
 * these calls evaluate it, term by term, on the device -- the one number that says how good the current level set is, which a caller
 * otherwise takes with cvh_get_levelset, cvh_get_image (8 + C bytes per pixel across PCIe) and a host pass.  The reference states the
 * functional and never evaluates it; the definition below IS the contract.  For the context's CURRENT level set u (h x w), its planes
 * I_k and its parameters (cvh_params: mu, nu, eps, lambda1, lambda2), everything in FP64:
 *     H_eps(x) = 1/2 (1 + (2/pi) atan(x / eps)),  delta_eps(x) = eps / (pi (eps^2 + x^2))             (src/main.cpp:188-210)
 *     gx(r, c) = (u(r, min(c + 1, w - 1)) - u(r, max(c - 1, 0))) * 0.5,  gy the same along the rows: central differences, replicate border
 *     length     = sum delta_eps(u) sqrt(gx^2 + gy^2)
 *     area       = sum H_eps(u)
 *     fit_in[k]  = sum (I_k - c1_k)^2 H_eps(u)
 *     fit_out[k] = sum (I_k - c2_k)^2 (1 - H_eps(u))
 *     total      = mu length + nu area + (1/C) sum_k (lambda1_k fit_in[k] + lambda2_k fit_out[k])
 * every sum over all h w pixels.  c1_k / c2_k are exactly the values cvh_get_means returns for this level set -- whatever it returns for
 * a nearly or wholly empty region included -- and come back in c1[] / c2[].  The host combines `total` from the term sums in exactly
 * the order written, left to right, k ascending.  Entries of the arrays behind the context's channel count are 0.  With "state" = 32
 * the level set is the one the getters see: the exact doubles of the float state.  A non-finite u gives non-finite terms; that is not
 * an error.
 * Determinism: the value of every term depends on the inputs and the member's shape alone -- not on the grid a batch gives the member,
 * not on the order workgroups arrive in, not on the other members.  Two calls in a row, and a member alone or inside any batch, give
 * the same bits.  (How: chan_vese_amd/csrc/energy_kernels.hip -- per-item partial sums in a fixed order, then one fixed-order
 * reduction per member; no atomics.)
 * The calls only READ: level set, run state, sums, options and planes are untouched; iterations in flight are settled first, as the
 * getters do; a run continued after the call is bit-identical to one without it.  Where the context's state block does not hold the
 * means of the current level set (a level set just arrived, planes or eps changed), they are taken inside the call, beside the run's
 * state and not into it.
 * cvh_energy_batch takes n contexts of any mix of shapes and channel counts on one device and writes out[0 .. n-1]: one set of launches
 * (term pass, reduce pass) on member 0's stream, ordered after everything already enqueued on the stream of every member and before
 * anything enqueued on them later, one host wait per call.  cvh_energy is the same path with n = 1.
 * Cost, one run of tools/energy_probe.py on an MI355X (host clock around a call and its wait, 20 calls): 72 / 80 / 149 us
 * at 1024^2 / 2048^2 / 4096^2, 198 us at 4096^2 x 3 -- about 70 us of it fixed (table upload, two launches, copy back, wait), and 2.2 to
 * 2.5 CSV iterations of the same plane at 4096^2; up to a third more where the means are taken inside the call.
 * CVH_ERR_ARG: a NULL list, member or out, n < 1, a context listed twice, contexts on different devices, h*w >= 2^32.  CVH_ERR_STATE: a
 * member without an image or without a level set.  Every member is checked before anything is launched; the message names the member
 * index and is cvh_last_error(NULL)'s (and the leader's); the contexts stay usable. */
typedef struct cvh_energy_terms {
  double total, length, area;
  double fit_in[CVH_MAX_CHANNELS], fit_out[CVH_MAX_CHANNELS];
  double c1[CVH_MAX_CHANNELS], c2[CVH_MAX_CHANNELS];
} cvh_energy_terms;
int cvh_energy(cvh_context *ctx, cvh_energy_terms *out);
int cvh_energy_batch(cvh_context *const *ctxs, int n, cvh_energy_terms *out);

/* ---- Mask scores ------------------------------------------------------------------------------------------------------------
 * How far the current segmentation is from a ground-truth mask, on the device: overlap (IoU, Dice) and boundary measures (Hausdorff
 * distance, average symmetric surface distance, surface Dice at a tolerance) -- what a caller otherwise takes with cvh_get_mask (one
 * byte per pixel across PCIe), a host pass and a Euclidean distance transform.  Everything is defined in INTEGERS, so every field of
 * cvh_mask_score is exact and can be compared with ==; no result depends on the grid, the schedule or the batch.
 * Masks.  For a context of h x w and a truth plane t of h x w bytes, row-major:
 *     M(p) = (((float)u(p) > 0) != invert)    cvh_get_mask's rule: NaN, -0.0 and a positive double that rounds to 0.0f are outside;
 *                                             with "state" = 32 the class comes from the float state, as in cvh_reinit / cvh_components
 *     T(p) = (t(p) != 0)
 * Overlap.  tp, fp, fn, tn count the pixels with (M, T) = (1,1), (1,0), (0,1), (0,0).
 * Surface.  surf(S) is the set of pixels of S with a 4-neighbour that is not in S; a neighbour outside the plane counts as not in S, so a
 * foreground pixel in the first or last row or column is always surface (S & ~binary_erosion(S, cross, border_value = 0)).  surf_m and
 * surf_t are the sizes of surf(M) and surf(T).
 * Distances.  For p in surf(M), d2_m(p) is the minimum over q in surf(T) of the squared pixel distance (row difference^2 + column
 * difference^2), an exact integer; d2_t(p) for p in surf(T) is the same against surf(M).
 *     q16(d2) = llrint(sqrt((double)d2) * 65536)     an IEEE sqrt, an exact multiply by 2^16, a round-half-even: 16.16 fixed point
 *     hd2_m, hd2_t             the maximum of d2_m / d2_t over its surface: the two directed Hausdorff distances, squared
 *     dist_m_q16, dist_t_q16   the sum of q16(d2) over the surface
 *     within_m, within_t       the surface pixels with d2 <= tol2 (tol2: the call's squared tolerance in pixels)
 *     defined                  1 when both surfaces are non-empty, else 0: then the six distance fields are 0, the overlap and surface
 *                              counts are still valid, and the call succeeds
 * Bounds: h^2 + w^2 < 2^32 and h w < 2^31; under them a 16.16 term is at most 2^32 and the sums cannot overflow 64 bits.
 * Derived figures (host arithmetic in doubles; chan_vese_amd/capi.py Score implements them once):
 *     iou = tp / (tp + fp + fn)                 dice = 2 tp / (2 tp + fp + fn)
 *     hausdorff = sqrt(max(hd2_m, hd2_t))       assd = (dist_m_q16 + dist_t_q16) / 65536 / (surf_m + surf_t)
 *     surface_dice = (within_m + within_t) / (surf_m + surf_t)
 * each NaN where its denominator is 0 or, for the last three, `defined` is 0.
 * Determinism: the sums are integers, combined by 64-bit adds and 32-bit maxima (vector atomics, one per workgroup and field): a member
 * alone or inside any batch, and two calls in a row, give the same bits (chan_vese_amd/csrc/score_kernels.hip).
 * cvh_score_mask takes host bytes: they are staged into the context's workspace and the device path runs.  cvh_score_mask_device and
 * cvh_score_mask_device_batch take device pointers under the rules of "Device-memory input and output": any byte alignment, memory
 * that kernels on the context's device can address, ordered behind what `stream` holds at the call.  The batch form serves n contexts of
 * one device, any mix of shapes and channel counts, and writes out[0 .. n-1]: ONE set of launches on member 0's stream, joined with
 * every member's stream before and after, and ONE host wait, for the result rows (the truth planes have been read when the call
 * returns).  The single forms are the same path with n = 1.
 * The calls only READ the level set: iterations in flight are settled first and the FP64 mirror of a float state is refreshed, as the
 * getters do; level set, run state, sums, options and planes are untouched, and a run continued after the call is bit-identical to one
 * without it.  An image is not required.  A context's first call allocates its workspace (5.5 bytes per pixel), kept until cvh_destroy.
 * Cost, one run of tools/score_probe.py on an MI355X (host clock around a call and its wait, 20 calls, measured once):
 * 142 / 999 / 512 us at 1024^2 / 2048^2 / 4096^2 for a noisy disk after 50 iterations against the clean disk -- the cost follows the
 * number of surface pixels and the length of their searches, not the plane -- beside 116 / 458 / 1712 ms for the same integers from
 * cvh_get_mask, numpy and scipy's distance transform.
 * CVH_ERR_ARG: out, truth or d_truths NULL or a NULL entry of d_truths; a pointer that is not device-accessible memory of the context's
 * device; ctxs NULL, n < 1, a NULL or duplicate member, members on different devices; a plane beyond the bounds.  CVH_ERR_STATE: a member
 * without a level set.  Every member is checked before anything is launched and `out` is written only by a call that succeeds; the
 * message names the member index and is cvh_last_error(NULL)'s (and member 0's). */
typedef struct cvh_mask_score {
  uint64_t tp, fp, fn, tn, surf_m, surf_t, within_m, within_t, dist_m_q16, dist_t_q16;
  uint32_t hd2_m, hd2_t; int32_t defined, pad;
} cvh_mask_score;
int cvh_score_mask(cvh_context *ctx, const uint8_t *truth, int invert, uint32_t tol2, cvh_mask_score *out);              /* host bytes */
int cvh_score_mask_device(cvh_context *ctx, const uint8_t *d_truth, int invert, uint32_t tol2, cvh_mask_score *out, void *stream);
int cvh_score_mask_device_batch(cvh_context *const *ctxs, int n, const uint8_t *const *d_truths, int invert, uint32_t tol2,
                                cvh_mask_score *out, void *stream);

/* ---- Component overlaps -------------------------------------------------------------------------------------------------------
 * "Mask scores" compares the mask with a ground-truth MASK; these calls relate the mask's OBJECTS to another set of objects: an instance
 * ground truth (per-object IoU, detections at an IoU threshold, precision, recall, F1, the threshold-averaged precision of the
 * cell-segmentation benchmarks), the components of the previous frame (cvh_components writes a device label plane: frame-to-frame
 * correspondence), or any labelling in which splits and merges are to be found.  All of it is read off one integer object, the
 * CONTINGENCY TABLE of two labelings -- what a caller otherwise takes by fetching 4 bytes of labels per pixel across PCIe and running
 * np.unique over h w pairs on a CPU.  Every field is an integer count: every row can be compared with ==.
 * For a context of h x w:
 *     A(p)    the label cvh_components gives pixel p on the mask cvh_get_mask_clean defines for (conn, invert, min_area, fill_holes,
 *             keep_largest) -- with (0, 0, 0) the raw mask of cvh_get_mask, exactly the arguments of cvh_measure: 0 is background,
 *             1 .. K are the components, numbered by their smallest flat index AFTER cleaning;
 *     B(p)    the caller's plane of h x w int32_t, row-major.  Any 32-bit value is allowed, negative ones included; the device treats it
 *             as opaque, and only the derived figures below read B == 0 as "no object";
 *     table   one row cvh_overlap { a, b, count, pad = 0 } (16 bytes) for every pair with count = #{p : A(p) = a, B(p) = b} > 0.  The
 *             pairs with a = 0 or b = 0, and (0, 0), are included;
 *     order   by a ascending, then by b ascending as a signed int32_t;
 *     P       the number of rows.  The counts add up to h w, and the area of component a is the sum of its rows (cvh_components' and
 *             cvh_measure's area is the cross-check).
 * Bound: h w < 2^31, so a count fits 32 bits.
 * Determinism: integer adds are order-free and the order of the rows is the sort's, not the schedule's: a member alone or inside any
 * batch, and two calls in a row, give the same P and the same bytes.
 * cvh_overlaps takes the plane from host memory: it is staged into the context (4 bytes per pixel) and the device path runs.
 * cvh_overlaps_device and cvh_overlaps_device_batch take device pointers under the rules of "Device-memory input and output": memory
 * that kernels on the context's device can address, aligned to 4 bytes as d_labels is, ordered behind what `stream` holds at the call
 * (the tensors cvh_components wrote for the previous frame qualify as they are).  `table` is HOST memory of `cap` rows, like
 * cvh_components' table; it may be NULL, and so may `tables` or any entry of it (caps is read only for the members with a table).
 * *pairs is always the full P, the table receives the first min(P, cap) rows in the defined order, *count is K; pairs, count and their
 * arrays may be NULL.  The batch form serves n contexts of one device, any mix of shapes and channel counts, with ONE set of launches
 * on member 0's stream, joined with every member's stream before and after as cvh_components_batch; the single forms are the same
 * kernels with n = 1.
 * The calls only READ: iterations in flight are settled first and the FP64 mirror of a float state is refreshed, as the getters do;
 * level set, run state, sums, options and planes are untouched, and a run continued after the call is bit-identical to one without.
 * An image is not required.
 * How (chan_vese_amd/csrc/overlap_kernels.hip): the cleaning and numbering launches of cvh_measure on the components workspace; then a
 * workgroup streams 8192 pixels of A and B in raster order, once, at 8 bytes per pixel; a lane forms the 64-bit key (a, b); the first
 * lane of every run of equal keys inside a wave adds the run's length to a 512-slot table in LDS (open addressing, at most 8 probes;
 * beyond them straight to global memory), and every occupied LDS slot goes once to the member's global open-addressing table: a key is
 * claimed by a 64-bit compare-and-swap against the empty key (whose a-half is -1), the count added by a 32-bit add, plain vector atomics
 * at agent scope.  A plane that is one pair -- the contended case -- costs one global atomic per workgroup.  Every probe loop is bounded
 * by the table's size and no workgroup waits for another: a table more than half full sets an overflow word, the remaining inserts are
 * dropped, and the host runs the pair launch again for that member on a table four times as large.  The table keeps its size in the
 * context, so the growth is paid once.  A last launch compacts the occupied slots into rows (one atomic per wave); they come down
 * unsorted and are SORTED ON THE HOST behind the wait for them (std::sort on 16-byte rows; P is the number of pairs, not of pixels).
 * Host waits: ONE for K, P and the overflow words; ONE MORE per growth of a member's table (none once the context's table has grown to
 * its content); and ONE MORE where any rows are asked for and P > 0 (P decides how many bytes come down).
 * Memory: the components workspace (8 bytes per pixel), cvh_get_mask's byte per pixel where the mask is cleaned, 4 bytes per pixel in
 * the host form, and 24 bytes per slot of the pair table: 4096 slots (96 KiB) at first, four times as many after each overflow, so at
 * most 8 P + 8 slots in use -- and in the worst case, every pixel its own pair, the first power of two above 2 h w: at most 96 bytes
 * per pixel.  Allocated on first use, kept until cvh_destroy; cvh_create allocates none of it.
 * Cost, one run of tools/overlap_probe.py on an MI355X (host clock around a call with a full table, its waits and the
 * sort, 20 calls, measured once): at 4096^2, a noisy disk after 50 iterations (350 components) against the clean disk's labels (P = 351)
 * 527 us, against a grid of 32 x 32 squares (P = 16975) 1628 us, of which about 1.0 ms are the rows' compaction, wait, fetch and sort
 * together (the count alone: 578 us); the plane wholly inside 651 / 1703 us; beside 73 - 126 ms for the same rows from cvh_components
 * with a label plane, a fetch and np.unique.  One case loses: at 1024^2 the same disk is still 90602 components, P = 90604, and the full
 * table takes 7.0 ms beside 6.7 ms the old way (the count alone 0.5 ms): with P near h w the fetch and the host's sort are the call.
 * CVH_ERR_ARG: what cvh_get_mask_clean refuses for conn, min_area, fill_holes and keep_largest; other or d_others NULL or a NULL entry
 * of d_others; a pointer that is not device-accessible memory of the context's device or not aligned to 4 bytes; a negative cap of a
 * member with a table; ctxs NULL, n < 1, a NULL or duplicate member, members on different devices; h w >= 2^31.  CVH_ERR_STATE: a member
 * without a level set.  Every member is checked before anything is launched, and the outputs are written only by a call that succeeds;
 * the message names the member index and is cvh_last_error(NULL)'s and member 0's.
 * cvh_match_overlaps (host only, no device, no context) derives the object-level counts from a table of `pairs` rows at the IoU
 * threshold num / den:
 *     objects_a, objects_b   the number of distinct a != 0, of distinct b != 0
 *     area_a, area_b         the sum of the counts of the rows with that a, with that b
 *     match                  a pair (a != 0, b != 0) matches when count den > num (area_a + area_b - count) in 64-bit unsigned arithmetic:
 *                            IoU strictly above num / den
 *     tp                     the number of matches; fp = objects_a - tp, fn = objects_b - tp
 * The call requires 0 < den <= 65535 and den <= 2 num <= 2 den: with IoU > 1/2 an a matches at most one b and a b at most one a (two
 * disjoint sets cannot each hold more than half of a third), so NO ASSIGNMENT PROBLEM arises and the matches are read off the rows.
 * match_of_a may be NULL; otherwise it holds k >= the largest a entries, and entry a - 1 receives the b that a matched, or 0.
 * Derived figures (host arithmetic in doubles; chan_vese_amd/capi.py ObjectScore implements them once):
 *     precision = tp / (tp + fp)      recall = tp / (tp + fn)      f1 = 2 tp / (2 tp + fp + fn)      ap = tp / (tp + fp + fn)
 *     mean_ap   the mean of ap over num / den = 10/20, 11/20 .. 19/20
 * each NaN where its denominator is 0.
 * CVH_ERR_ARG: out NULL, table NULL with pairs > 0, pairs < 0; a threshold outside the range above; a table that is not in the defined
 * order (a pair twice included), has a zero count or a negative a; k smaller than the largest a (with match_of_a). */
typedef struct cvh_overlap { int32_t a, b; uint32_t count, pad; } cvh_overlap;   /* 16 bytes */
typedef struct cvh_match { uint32_t objects_a, objects_b, tp, fp, fn, pad; } cvh_match;
int cvh_overlaps(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                 const int32_t *other /* host */, cvh_overlap *table, long cap, long *pairs, int *count);
int cvh_overlaps_device(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                        const int32_t *d_other, cvh_overlap *table, long cap, long *pairs, int *count, void *stream);
int cvh_overlaps_device_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                              const int32_t *const *d_others, cvh_overlap *const *tables, const long *caps, long *pairs, int *counts,
                              void *stream);
int cvh_match_overlaps(const cvh_overlap *table, long pairs, uint32_t num, uint32_t den, int32_t *match_of_a, int k,
                       cvh_match *out);   /* host only */

/* ---- Component measures -------------------------------------------------------------------------------------------------------
 * "Connected components of the mask" labels, boxes and cleans; these calls MEASURE: per component where it is, how large, how
 * elongated and how bright -- what a caller otherwise takes with cvh_get_mask, cvh_get_image (both across PCIe) and a pass of
 * scipy.ndimage / skimage.regionprops on a CPU.  Every field of cvh_region is a sum (or a minimum / maximum) of INTEGERS: a member alone
 * or inside any batch, and two calls in a row, give the same bits, and every field can be compared with ==.
 * The mask measured is the one cvh_get_mask_clean defines for (conn, invert, min_area, fill_holes, keep_largest) -- with (0, 0, 0) the
 * raw mask of cvh_get_mask --, labelled with `conn` in cvh_components' numbering: row k-1 describes label k.  With (0, 0, 0) the
 * fields first, area, x0 .. y1 are cvh_components' table byte for byte.  Over the pixels p = (row r, column c) of label k:
 *     first, area, x0, y0, x1, y1   as cvh_component
 *     border      the number of the component's pixels in the first or last row or column
 *     perimeter   the number of pixel edges of the component's pixels whose 4-neighbour across the edge is background or lies outside
 *                 the plane (a foreground 4-neighbour always belongs to the same component, for either conn)
 *     sx = sum c, sy = sum r, sxx = sum c^2, syy = sum r^2, sxy = sum r c
 *     s1[k] = sum I_k(p), s2[k] = sum I_k(p)^2   over the context's C planes as they are now (after cvh_perona_malik: the smoothed
 *                 planes), the bytes cvh_histogram reads; the entries of channels >= C are 0
 *     reserved    0
 * Bounds: h <= 65535, w <= 65535 and h w < 2^31; under them sxx, syy and sxy stay below 2^31 2^32 = 2^63 and every other sum far
 * below that.
 * cvh_region_shape_of (host only, no device, no context) derives the usual figures from a row, with A = area:
 *     cx = (double)sx / (double)A, cy likewise
 *     mu20 = (double)(A sxx - sx^2) / ((double)A (double)A)   the numerator an exact 128-bit integer, converted ONCE with round to
 *                 nearest even; mu02 the same from syy and sy, mu11 the same from the signed A sxy - sx sy
 *     mean[k] = (double)s1[k] / (double)A,  var[k] = (double)(A s2[k] - s1[k]^2) / ((double)A (double)A)    for k < channels, else 0
 *     theta = 0.5 atan2(2 mu11, mu20 - mu02)
 *     major, minor = 4 sqrt(l+), 4 sqrt(l-) with l+- = (mu20 + mu02) / 2 +- sqrt(((mu20 - mu02) / 2)^2 + mu11^2); minor is 0 where l-
 *                 rounds below 0
 * Everything up to and including var is IEEE arithmetic on exact integers (Python's float(int) arithmetic reproduces it bit for bit);
 * theta, major and minor go through libm.  CVH_ERR_ARG: area == 0, a NULL pointer, channels not 1 or 3.
 * cvh_measure: table (host, cap rows) may be NULL, count may be NULL.  *count is always the full K; table receives the first
 * min(K, cap) rows.  cvh_measure_batch: tables may be NULL and so may any of its entries (no rows for that member; caps is read only
 * for the members with a table); counts is an array of n or NULL.  A member with K = 0 is no error.  The batch form serves n contexts
 * of one device, any mix of shapes and channel counts, with ONE set of launches on member 0's stream, joined with every member's
 * stream before and after as cvh_components_batch; cvh_measure is the same kernels with n = 1.  `stream`: the call is ordered behind
 * what it holds at the call.
 * Host waits: ONE for the counts, and a SECOND where any rows are asked for (K decides where the rows live; they are computed behind
 * the first wait).
 * The calls only READ: iterations in flight are settled first and the FP64 mirror of a float state is refreshed, as the getters do;
 * level set, run state, sums, options and planes are untouched, and a run continued after the call is bit-identical to one without.
 * How (chan_vese_amd/csrc/measure_kernels.hip): the forest, flatten, count, scan and number launches of cvh_components (for a cleaned
 * mask: the launches of cvh_get_mask_clean into the context's own mask buffer, labelled from its bytes); then a workgroup takes 8192
 * pixels in raster order, forms the sums of every horizontal run inside a wave (a segmented reduction for perimeter, border, s1 and
 * s2; closed forms of row, first column and length for the others), combines the runs of a label in a small label -> sums cache in LDS,
 * and sends a cached row to the global row with 64-bit atomics only when another label takes its slot and once at the end: a plane
 * that is one component costs one set of atomics per workgroup, not per run.
 * Cost, one run of tools/measure_probe.py on an MI355X (host clock around a call with a full table and its two waits,
 * 20 calls, measured once): 680 us at 4096^2 for a noisy disk after 50 iterations (350 components), 1130 us for the plane wholly inside
 * (one component: 1.7 x, the contention is cut, not gone), beside 331 / 1140 ms for the same rows from cvh_get_mask, cvh_get_image and numpy.
 * Memory: the components workspace (8 bytes per pixel), cvh_get_mask's byte per pixel where the mask is cleaned, and 128 bytes per row
 * asked for; allocated on first use, kept until cvh_destroy.
 * CVH_ERR_ARG: what cvh_get_mask_clean refuses for conn, min_area, fill_holes and keep_largest; a negative cap; ctxs NULL, n < 1, a
 * NULL or duplicate member, members on different devices; h > 65535, w > 65535 or h w >= 2^31.  CVH_ERR_STATE: a member without an image
 * or without a level set.  Checked for every member before anything is launched; the message names the member index and is
 * cvh_last_error(NULL)'s and member 0's. */
typedef struct cvh_region {            /* 128 bytes */
  uint32_t first, area; int32_t x0, y0, x1, y1;   /* exactly cvh_component's fields */
  uint32_t border, reserved;
  uint64_t perimeter, sx, sy, sxx, syy, sxy;
  uint64_t s1[3], s2[3];
} cvh_region;
typedef struct cvh_region_shape { double cx, cy, mu20, mu02, mu11, theta, major, minor, mean[3], var[3]; } cvh_region_shape;

int cvh_measure(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                cvh_region *table, int cap, int *count, void *stream);
int cvh_measure_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                      cvh_region *const *tables, const int *caps, int *counts, void *stream);
int cvh_region_shape_of(const cvh_region *r, int channels, cvh_region_shape *out);   /* host only */

/* ---- Contours -----------------------------------------------------------------------------------------------------------------
 * The boundary of the mask as ORDERED CLOSED LOOPS of lattice points -- what cv::findContours gives, and what a caller otherwise takes
 * with cvh_get_mask (a byte per pixel across PCIe) and a tracer on a CPU.  (cvh_get_contour is something else: a byte map of painted
 * pixels.)  Everything is defined in integers: a member alone or inside any batch, and two calls in a row, give the same bits, and every
 * field can be compared with ==.
 * Mask.  f(p) is the foreground of cvh_get_mask_clean for the call's (conn, invert, min_area, fill_holes, keep_largest); with
 * (., ., 0, 0, 0) it is cvh_get_mask's rule and the labelling launches do not run.  With "state" = 32 the class comes from the float
 * state, as everywhere else.
 * Lattice.  Vertices are (x, y) with 0 <= x <= w and 0 <= y <= h; pixel (row r, column c) is the square [c, c+1] x [r, r+1].
 * Edges.  A boundary edge is a side of a foreground pixel whose neighbour across it is not foreground or lies outside the plane.  Its
 * id is 4 (r w + c) + k.  Edges are directed so that the foreground is on the right (y grows downwards):
 *     k = 0 top     (c, r)     -> (c+1, r)          k = 1 right   (c+1, r)   -> (c+1, r+1)
 *     k = 2 bottom  (c+1, r+1) -> (c, r+1)          k = 3 left    (c, r+1)   -> (c, r)
 * Successor.  The successor of an edge is the boundary edge that leaves its head vertex; where two leave (two foreground pixels meet
 * diagonally) it is the left turn for conn = 8 and the right turn for conn = 4.  Every edge then has exactly one successor and one
 * predecessor: the edges fall into disjoint cycles.
 * Loop.  A loop is one cycle.  first is its smallest edge id, edges its length, area2 = sum (x_tail y_head - x_head y_tail) over its
 * edges -- twice the enclosed area, positive for an outer boundary, negative for a hole.  Loops are numbered in increasing order of
 * first.  The pixel first >> 2 is a foreground pixel on the loop: its label in cvh_components' label plane names the component.
 * Points.  With simplify = 0 a loop's points are the tail vertices of its edges in cycle order, starting at edge first.  With
 * simplify = 1 only corners stay -- a corner is the tail of an edge whose predecessor has another direction --, in the same order,
 * starting at the first corner met from edge first, that edge included.  points is their number, offset the loop's first index in the
 * point array: loop k's points follow loop k-1's.  A point is two int32, x then y.
 * Caps.  *nloops and *npoints are always the full counts; the loop table receives the first min(nloops, loop_cap) rows, the point
 * array the points with index < point_cap; nothing behind is written.  Either output may be NULL (counts only; no member with a point
 * array: the scatter launch is skipped), and so may nloops and npoints.  An empty mask gives 0 loops: no error.
 * cvh_contours writes the points to host memory, cvh_contours_device to device memory the caller owns (the rules of "Device-memory input
 * and output"; 4-byte aligned), ordered against `stream` by events: behind what it holds at the call, and it waits for the points.
 * The loop table is host memory in every form.  cvh_contours_device_batch serves n contexts of one device, any mix of shapes and
 * channel counts: loops, d_points and their entries may be NULL, the caps are read for the members with an output, nloops and npoints
 * are arrays of n or NULL; ONE set of launches on member 0's stream, joined with every member's stream before and after as
 * cvh_reinit_batch.  The single forms are the same kernels with n = 1.
 * The calls only READ: iterations in flight are settled first and the FP64 mirror of a float state is refreshed, as the getters do;
 * level set, run state, sums, options and planes are untouched, and a run continued after the call is bit-identical to one without.
 * How (chan_vese_amd/csrc/contour_kernels.hip): the mask bytes (the mask kernel, or the launches of cvh_get_mask_clean); per pixel the
 * 4-bit set of its boundary edges, counted per workgroup and scanned -- E, the number of edges; then, over the E edges in the order of
 * their ids: successor links, ceil(log2 E) rounds of pointer doubling (one launch each, double-buffered, ordered by kernel boundaries)
 * that give every edge its loop's smallest edge and the points between itself and it; the heads counted and scanned (the loop index);
 * edges, points and area2 per loop by integer atomics behind a reduction inside the wave; a scan of the points (offset); the scatter.
 * No kernel waits for another workgroup.
 * Host waits: TWO -- for the edge counts (they size the per-edge workspace, the grids and the rounds), then for the loop and point
 * counts and the rows.  A call whose masks are all empty ends at the first.
 * Memory: 6 bytes per pixel (mask, edge sets, prefix words), allocated by a context's first call; 45 bytes per edge, grown to the
 * largest E the context has met (plus a quarter); the host form also 8 bytes per point asked for; with cleaning, the components
 * workspace (8 bytes per pixel).  All kept until cvh_destroy; cvh_create allocates none of it.
 * Cost, one run of tools/contour_probe.py on an MI355X (host clock around a call with full outputs and its two waits, 20
 * calls, measured once): 1023 / 904 / 1223 us at 1024^2 / 2048^2 / 4096^2 for a noisy disk after 50 iterations, 593 / 741 / 1266 us for
 * the plane wholly inside (one loop) -- about twenty CSV iterations at 4096^2, nearly all of it launches, waits and scans that a call
 * without outputs pays too; cvh_get_mask alone takes 0.2 to 2 ms.
 * CVH_ERR_ARG: what cvh_get_mask_clean refuses for conn, min_area, fill_holes and keep_largest; simplify not 0 or 1; a negative cap;
 * h w >= 2^30 (an edge id is 32 bits); a point pointer that is not device-accessible memory of the context's device or not 4-byte
 * aligned; ctxs NULL, n < 1, a NULL or duplicate member, members on different devices; tables without caps.  CVH_ERR_STATE: a member
 * without a level set.  Checked for every member before anything is launched; the message names the member index and is
 * cvh_last_error(NULL)'s and member 0's. */
typedef struct cvh_contour_loop {      /* 32 bytes */
  uint32_t first, edges, points, pad;
  uint64_t offset;
  int64_t  area2;
} cvh_contour_loop;
int cvh_contours(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest, int simplify,
                 cvh_contour_loop *loops, long loop_cap, int32_t *points, long point_cap, long *nloops, long *npoints);   /* host points */
int cvh_contours_device(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest, int simplify,
                        cvh_contour_loop *loops, long loop_cap, int32_t *d_points, long point_cap, long *nloops, long *npoints,
                        void *stream);
int cvh_contours_device_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                              int simplify, cvh_contour_loop *const *loops, const long *loop_caps, int32_t *const *d_points,
                              const long *point_caps, long *nloops, long *npoints, void *stream);

/* ---- Subpixel contours --------------------------------------------------------------------------------------------------------
 * The ZERO LEVEL of the level set as ordered closed POLYGONS with subpixel vertices: the loops of "Contours", each lattice point
 * replaced by the point where u changes sign across the loop's edge.  A lattice point lies up to half a pixel from the zero level; these
 * lie on it to within the curvature of u inside a pixel.  What a caller otherwise does with cvh_get_levelset (8 bytes per pixel across
 * PCIe) and a marching-squares tracer on a CPU.
 * Why no new tracing: a boundary edge of the mask separates a foreground pixel from a background pixel (or the plane's border); the
 * segment that joins the two pixel centres carries exactly one marching-squares vertex; so a loop's edges in their cycle order ARE the
 * vertices of the marching-squares polygon in order, and the diagonal ambiguity is settled by conn as in "Contours".
 * Mask, loops, edges, successor rule.  Exactly those of "Contours" for the call's (conn, invert, min_area, fill_holes, keep_largest).
 * The loop table is the one cvh_contours writes with simplify = 0: points == edges, offset is the prefix of edges, area2 is the LATTICE
 * loop's.
 * One point per edge.  A loop's points are in cycle order and start at edge first.  For edge id 4 (r w + c) + k:
 *     p = (r, c) is the foreground pixel, q its neighbour across side k;
 *     (dx, dy) = (0, -1) for k = 0 (top), (1, 0) for k = 1 (right), (0, 1) for k = 2 (bottom), (-1, 0) for k = 3 (left);
 *     s = invert ? -1 : +1;  a = s u(p), b = s u(q) as FP64 (with "state" = 32 the floats widened, which is exact);
 *     t = a / (a - b), one IEEE division, when q lies inside the plane AND a > 0 AND b <= 0 AND a - b is finite; otherwise t = 0.5 --
 *         a plane-border edge; a pixel whose class was changed by cleaning; NaN, zeros of either sign, or a positive double that rounds
 *         to 0.0f (background by the mask's rule); an infinite a; an overflowing difference.  So t lies in [0, 1];
 *     x = (c + 0.5) + dx t,  y = (r + 0.5) + dy t, one rounding each: pixel centres are at half-integers, in the lattice of "Contours".
 * A point is two doubles, x then y.  Every bit is defined: the result can be compared with == against a numpy restatement, and a member
 * gives the same bits alone or in any batch (the library is built without floating-point contraction and without fast-math).
 * Caps, NULL outputs, empty masks, host waits, stream ordering, the batch form: as "Contours".  A point is 16 bytes; a device pointer
 * must be 8-byte aligned; the host form takes 16 bytes per point asked for on the device.  No new per-edge or per-pixel workspace: the
 * last launch of the trace is another scatter (a gather of u(p) and u(q) per edge, one 16-byte store), everything before it is the
 * integer path's.
 * The calls only READ, as cvh_contours: iterations in flight are settled, the FP64 mirror of a float state is refreshed, and a run
 * continued afterwards is bit-identical to one without.
 * After cvh_reinit every point is its edge's MIDPOINT: the distance to a pixel-edge front gives a = 0.5 and b = -0.5 on every edge.  The
 * subpixel position lives in the evolved u, not in a reinitialised one -- take the polygon before reinitialising.
 * cvh_contour_subpixel_measure (host only; no device, no context): for the n points of ONE loop
 *     area = 1/2 sum (x_i y_{i+1} - x_{i+1} y_i),   length = sum sqrt((x_{i+1} - x_i)^2 + (y_{i+1} - y_i)^2),   i = 0 .. n-1 cyclic,
 * each accumulated left to right in FP64 in index order, so that sequential double arithmetic reproduces it bit for bit; the sign is
 * area2's (positive for an outer boundary, negative for a hole).  n = 0 gives 0 and 0.  CVH_ERR_ARG: n < 0 or a NULL argument.
 * Cost, one run of tools/subpixel_probe.py on an MI355X (host clock around a call with full outputs and its two waits, 20
 * calls, measured once): 757 / 748 / 1009 us at 1024^2 / 2048^2 / 4096^2 for a noisy disk after 50 iterations, 410 / 536 / 1057 us for
 * the plane wholly inside -- beside 755 / 747 / 1054 and 412 / 535 / 1058 us for cvh_contours_device(simplify = 0) on the same level
 * sets in the same process: the two calls cannot be told apart (one gather of 16 bytes per edge beside about thirty launches).
 * CVH_ERR_ARG / CVH_ERR_STATE: what cvh_contours* refuses (there is no simplify), and a device point pointer that is not 8-byte
 * aligned. */
int cvh_contours_subpixel(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                          cvh_contour_loop *loops, long loop_cap, double *points, long point_cap, long *nloops, long *npoints);   /* host points */
int cvh_contours_subpixel_device(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                 cvh_contour_loop *loops, long loop_cap, double *d_points, long point_cap, long *nloops, long *npoints,
                                 void *stream);
int cvh_contours_subpixel_device_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                       cvh_contour_loop *const *loops, const long *loop_caps, double *const *d_points,
                                       const long *point_caps, long *nloops, long *npoints, void *stream);
int cvh_contour_subpixel_measure(const double *points, long n, double *area, double *length);   /* host only */

/* ---- Mask morphology ----------------------------------------------------------------------------------------------------------
 * Open, close, dilate or erode the mask by a disk ON THE DEVICE, and turn a byte mask into a level set there -- what a caller otherwise
 * does with cvh_get_mask, scipy.ndimage.binary_opening / cv::morphologyEx on a CPU, and cvh_set_levelset at 8 bytes per pixel.  Together
 * they close the loop segment -> clean or morph -> write back as the level set, after which cvh_components, cvh_measure, cvh_contours,
 * cvh_score_mask*, cvh_reinit and further iterations see the result.  Everything is defined in integers: a member alone or inside any
 * batch, and two calls in a row, give the same bytes, and every byte can be compared with ==.
 *   plane       P is the set of the plane's pixels;
 *   start set   F0 is the clean mask: exactly the set cvh_get_mask_clean gives for (conn, invert, min_area, fill_holes, keep_largest);
 *               with (., invert, 0, 0, 0) it is cvh_get_mask's.  With "state" = 32 the class comes from the float state, as elsewhere;
 *   disk        D(r2) = { (dx, dy) in Z^2 : dx^2 + dy^2 <= r2 } in 64-bit integers, r2 any uint32_t: r2 = 0 is the identity, r2 = 1 the
 *               4-neighbour cross, r2 = 2 the 3 x 3 square;
 *   dilate(F)   = { p in P : some d in D has p + d in F } -- p belongs iff the exact squared Euclidean distance from p to the nearest
 *               pixel of F is <= r2; an empty F gives an empty result;
 *   erode(F)    = { p in P : every d in D with p + d in P has p + d in F } = P \ dilate(P \ F);
 *   open(F)     = dilate(erode(F)), close(F) = erode(dilate(F));
 *   border      pixels outside the plane belong to neither set: only background pixels OF THE PLANE erode, so erosion and dilation are
 *               exact duals under complement.  In scipy's terms: binary_dilation(F, disk, border_value=0) and
 *               binary_erosion(F, disk, border_value=1);
 *   op          CVH_MORPH_NONE, _DILATE, _ERODE, _OPEN, _CLOSE; with CVH_MORPH_NONE, or with r2 = 0, the result is F0;
 *   mask start  given h*w bytes, u(p) = (byte(p) != 0) ? inside : outside;
 *   level sets  inside and outside are any doubles, NaN included, stored bit for bit.  Every call here that writes a level set leaves
 *               the context exactly as cvh_set_levelset of the same doubles would -- a new run, cleared counter, stop flag and sums, with
 *               "state" = 32 the float pair adopted --, done the way the cvh_init_* calls do it; iterations in flight are settled first.
 * cvh_get_mask_morph* only READ (as cvh_get_mask_clean*): a run continued after them is bit-identical to one without.  The output is a
 * 0/1 uint8 mask, in host memory or in device memory the caller owns.
 * cvh_morph_levelset* is IN PLACE: the level set becomes inside where that mask is 1 and outside elsewhere.  The morphed mask never
 * leaves the device and needs no caller buffer; with CVH_MORPH_NONE the call bakes the cleaned mask into the level set.
 * cvh_init_mask* needs neither an image nor a level set.  cvh_init_mask takes host bytes: 1 byte per pixel goes up, not 8.
 * Device pointers follow the rules of "Device-memory input and output" above (hipPointerGetAttributes check, any byte alignment, event
 * ordering against `stream`).  The *_batch forms serve n contexts of one device, any mix of shapes and channel counts, with ONE set of
 * launches on member 0's stream, joined with every member's stream before and after as cvh_get_mask_clean_device_batch and
 * cvh_init_checkerboard_batch; r2 is per member (an array of n), op is shared.  The single forms are the same kernels with n = 1.  A
 * member's output depends on its inputs and shape alone: no atomic and no floating-point sum is involved.
 * Host waits: cvh_get_mask_morph_device[_batch] NONE beyond what cvh_get_mask_clean_device makes (the caller's stream waits, the host
 * does not); cvh_get_mask_morph ONE, for its bytes, as cvh_get_mask_clean; cvh_morph_levelset[_batch] and cvh_init_mask* ONE, as
 * cvh_init_rect, behind which the members begin their new run.
 * How (chan_vese_amd/csrc/morph_kernels.hip): the start set packed into one word per band of 32 rows and column (from the level set,
 * or from the bytes the cleaning launches left); per pass a column launch -- each pixel's vertical distance to the nearest set pixel,
 * cut off at floor(sqrt(r2)), with the reinitialisation's fix-up across bands -- and a row launch that accepts pixel j iff some
 * |k| <= floor(sqrt(r2)) has k^2 + g(j + k)^2 <= r2 (a pixel of the set is accepted without a search) and packs the result again; an
 * erosion is the same pass on the complement within the plane; open and close are two passes; an emit launch writes bytes or level-set
 * doubles in 16-byte pieces.  The launches are ordered by kernel boundaries alone.
 * Memory: 3.25 bytes per pixel (two planes of band words, a 16-bit distance field, a byte plane for the cleaned mask or the host
 * form's bytes), allocated by a context's first call and kept until cvh_destroy; with cleaning, the components workspace as well.
 * cvh_create allocates none of it and the automatic choices that weigh the contexts of a device do not count it.
 * Cost, one run of tools/morph_probe.py on an MI355X (host clock around a call and its wait, 20 calls, measured once):
 * open / close of a noisy disk after 50 iterations at r2 = 2, 25, 400: 109 - 384 us at 1024^2, 126 - 418 us at 2048^2, 192 - 694 us at
 * 4096^2; cvh_init_mask_device 28 / 38 / 66 us.  cvh_get_mask + scipy + cvh_set_levelset took 15 ms to 9.1 s for the same bytes.
 * CVH_ERR_ARG: op outside 0 .. 4; what cvh_get_mask_clean refuses for conn, min_area, fill_holes and keep_largest; a NULL r2, mask or
 * pointer array; a pointer that is not device-accessible memory of the context's device; a plane with h^2 + w^2 >= 2^32 (cvh_reinit's
 * cap; cvh_init_mask*: h w >= 2^32); ctxs NULL, n < 1, a NULL or duplicate member, members on different devices.  CVH_ERR_STATE: the
 * morph calls on a member without a level set.  Checked for every member before anything is launched; the message names the member
 * index and is cvh_last_error(NULL)'s and member 0's. */
#define CVH_MORPH_NONE   0
#define CVH_MORPH_DILATE 1
#define CVH_MORPH_ERODE  2
#define CVH_MORPH_OPEN   3
#define CVH_MORPH_CLOSE  4
int cvh_get_mask_morph(cvh_context *ctx, uint8_t *mask, int conn, int invert, long min_area, long fill_holes, int keep_largest, int op,
                       uint32_t r2);   /* host bytes, 0/1 */
int cvh_get_mask_morph_device(cvh_context *ctx, uint8_t *d_mask, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                              int op, uint32_t r2, void *stream);
int cvh_get_mask_morph_device_batch(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, int conn, int invert, long min_area,
                                    long fill_holes, int keep_largest, int op, const uint32_t *r2, void *stream);
int cvh_morph_levelset(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest, int op, uint32_t r2,
                       double inside, double outside);
int cvh_morph_levelset_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                             int op, const uint32_t *r2, double inside, double outside);
int cvh_init_mask(cvh_context *ctx, const uint8_t *mask, double inside, double outside);   /* host bytes */
int cvh_init_mask_device(cvh_context *ctx, const uint8_t *d_mask, double inside, double outside, void *stream);
int cvh_init_mask_device_batch(cvh_context *const *ctxs, int n, const uint8_t *const *d_masks, double inside, double outside,
                               void *stream);

/* ---- Object split ---------------------------------------------------------------------------------------------------------------
 * Take touching objects apart ON THE DEVICE: erode, label, grow back, cut.  Every object-level call here (cvh_components, cvh_measure,
 * cvh_contours, cvh_overlaps, cvh_match_overlaps) takes one connected component for one object; where objects touch (cells, grains,
 * droplets) the mask holds one blob for two, and what a caller otherwise does is cvh_get_mask, a distance transform, a labelling and a
 * watershed on a CPU, and cvh_init_mask.  This is the classical "reconstruction by geodesic influence zones", not a grey-level watershed:
 * it is defined in integers, independent of schedule and grid, so a member alone or inside any batch, and two calls in a row, give the
 * same bytes, and every output can be compared with ==.
 * Given (conn, invert, min_area, fill_holes, keep_largest) and r2, any uint32_t:
 *   start set   F0 is the clean mask, exactly cvh_get_mask_clean's set; with (., invert, 0, 0, 0) it is cvh_get_mask's.  With "state" =
 *               32 the class comes from the float state, as elsewhere;
 *   eroded set  E = erode(F0) by the disk D(r2) of "Mask morphology": pixels outside the plane belong to neither set; r2 = 0 gives E = F0;
 *   markers     M = E  u  { p in F0 : the conn-component of F0 that holds p has no pixel in E }.  A component the erosion wipes out stays
 *               whole: it is its own marker, so nothing is ever lost.  The conn-components of M are numbered 1 .. K in increasing order
 *               of their smallest flat index -- cvh_components' numbering --, m(p) is that number for a pixel p of M;
 *   growth      for p in F0, d(p) is the length of the shortest conn-path inside F0 from p to M (d = 0 on M), and
 *                   L(p) = m(p) on M;   L(p) = min { L(q) : q a conn-neighbour of p in F0 with d(q) = d(p) - 1 } elsewhere in F0;
 *                   L = 0 outside F0;
 *   fixpoint    equivalently, with key(p) = (d(p), L(p)) compared lexicographically, the keys are the unique fixpoint of
 *                   key(p) = min(key(p), min over the conn-neighbours q of p in F0 of (d(q) + 1, L(q))),   key = (0, m(p)) fixed on M.
 *               The operator is monotone and keys only fall from (infinity, .), so every key stays an upper bound of the fixpoint and
 *               ANY order of relaxation -- synchronous, tile by tile, lanes racing, a neighbour's key read a sweep late -- ends in the
 *               same bits once no relaxation changes anything.  That is what lets the kernel iterate freely;
 *   reach       every pixel of F0 is reached: every component of F0 holds a marker;
 *   table       row k - 1 is a cvh_component for label k: first the smallest flat index of the MARKER, area and the inclusive box those
 *               of { p : L(p) = k }, cut pixels included;
 *   cut         cut(p) <=> L(p) > 0 and some 8-neighbour q of p has L(q) > L(p).  One-sided, so the lines are one pixel wide.  After the
 *               cut no two pixels of different labels are 8-adjacent: of such a pair the one with the smaller label sees a larger label
 *               beside it and is cut.  The pieces are therefore separate under either connectivity;
 *   unchanged   with r2 = 0, or with r2 so large that E is empty, M = F0: L is cvh_components' label plane of the clean mask and the table is
 *               cvh_components' table; the cut is empty (but, with conn = 4, between components that touch diagonally: the rule above
 *               holds them apart as well).  K = 0 on an all-background plane is not an error.
 * cvh_split only READS (as cvh_components): a run continued after it is bit-identical to one without.  d_labels (h w int32 in device
 * memory the caller owns, 4-byte aligned, the rules of "Device-memory input and output") may be NULL, and so may table (host, cap rows:
 * the first min(K, cap)) and count (always the full K).  cvh_split_batch serves n contexts of one device, any mix of shapes and channel
 * counts, with ONE set of launches on member 0's stream, joined with every member's stream before and after as cvh_components_batch; r2
 * is per member (an array of n); d_labels and its entries may be NULL, counts is an array of n or NULL.  cvh_split_host writes the labels to
 * host memory (not NULL): they are staged in the int32 plane of cvh_overlaps' host form (4 bytes per pixel, the context's) and come down
 * behind one more wait.
 * cvh_split_levelset[_batch] is IN PLACE: u = inside on F0 \ cut and outside elsewhere, any doubles, stored bit for bit; the context is
 * left exactly as cvh_set_levelset of those doubles would leave it, as cvh_morph_levelset does.  After it every mask-based call --
 * cvh_components, cvh_measure, cvh_contours, cvh_overlaps, cvh_score_mask*, cvh_reinit, further iterations -- sees the split objects.
 * Because the cut looks at 8 neighbours whatever conn is, cvh_split_levelset(r2 = 0, conn = 4) is NOT a no-op on a mask whose
 * 4-components touch diagonally: it cuts the smaller-labelled pixel of every such contact (with conn = 8 and r2 = 0 it changes no class).
 * How (chan_vese_amd/csrc/split_kernels.hip): F0 as bytes (the mask kernel, or cvh_get_mask_clean's launches); the erosion pass of
 * "Mask morphology"; the forest launches of cvh_components on F0's bytes; a flag per component "has an eroded pixel" (a vector atomic OR
 * on the component's root) and M as bytes; the numbering launches of cvh_components on M; then the growth.  A key is 64 bits,
 * (d << 32) | L: d < h w < 2^31 and L <= K <= 2^30 fit, so the cap is the labelling's.  A workgroup owns a tile of 32 x 64 keys plus a
 * one-pixel halo in LDS, relaxes it until it is stable, stores the keys that fell and adds their number to the member's counter; a
 * launch is one such sweep over all tiles of all members; no workgroup waits for another.  Sweeps are enqueued in groups of 4
 * (cvh_split_geometry): a sweep of a member whose sweep before changed nothing returns at once, and the host reads the counters once
 * per group.  One launch then takes the cut and writes labels or level-set doubles in 16-byte pieces; the single form's table is two
 * more launches on L.
 * Host waits: ceil(sweeps / 4), the first of which also brings the counts, and ONE more behind the outputs (labels, rows or level set;
 * none where only counts are asked for) -- cvh_components' one or two, plus the groups.  sweeps is 1 + the number of tile seams the
 * longest growth path crosses, give or take what racing workgroups pass on within a sweep: 4 to 6 in the fields measured below.   
 * Memory: 8 bytes per pixel of the plane rounded up to whole tiles (the keys), allocated by a context's first call and kept until
 * cvh_destroy, beside the morphology workspace (3.25 bytes per pixel) and the components workspace (8 bytes per pixel), which the calls
 * share with those families.  cvh_create allocates none of it.
 * The result depends on the radius: too small splits nothing, too large erodes small objects away (they stay whole), and in between a
 * neck can leave a spurious sliver as a core of its own (README.md shows one).  The radius is the caller's choice; nothing here picks it.
 * Cost, one run of tools/split_probe.py on an MI355X (host clock around a call with a label plane, a full table and its
 * waits, 20 calls, measured once): a field of touching disks built so that every case splits, R = 4 / 16 / 64: 1.5 / 1.3 / 3.0 ms at 1024^2,
 * 2.2 / 1.9 / 3.5 ms at 2048^2, 5.9 / 4.8 / 6.9 ms at 4096^2 with 4 to 6 sweeps; a speckled mask with nothing to grow 0.88 / 2.96 / 10.7 ms
 * beside 0.77 / 2.74 / 9.9 ms for cvh_components with its table.  cvh_get_mask + the numpy restatement + cvh_init_mask took 65 - 3458 ms at
 * 1024^2 for the same labels.
 * CVH_ERR_ARG: what cvh_get_mask_clean refuses for conn, min_area, fill_holes and keep_largest; a NULL r2 list; a negative cap; a label
 * pointer that is not device-accessible memory of the context's device or not 4-byte aligned; h^2 + w^2 >= 2^32 or h w >= 2^31; ctxs
 * NULL, n < 1, a NULL or duplicate member, members on different devices.  CVH_ERR_STATE: a member without a level set.  Checked for every
 * member before anything is launched; the message names the member index and is cvh_last_error(NULL)'s and member 0's. */
int cvh_split(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest, uint32_t r2, int32_t *d_labels,
              cvh_component *table, int cap, int *count, void *stream);
int cvh_split_host(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest, uint32_t r2, int32_t *labels,
                   cvh_component *table, int cap, int *count);   /* host labels */
int cvh_split_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                    const uint32_t *r2, int32_t *const *d_labels, int *counts, void *stream);
int cvh_split_levelset(cvh_context *ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest, uint32_t r2,
                       double inside, double outside);
int cvh_split_levelset_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                             const uint32_t *r2, double inside, double outside);
void cvh_split_geometry(int *tile_rows, int *tile_cols, int *group);   /* pure host arithmetic: the growth's tile and the sweeps per group */

/* ---- Four phases ----------------------------------------------------------------------------------------------------------------
 * Vese and Chan's multiphase model: TWO level sets evolved together, whose sign pairs name four regions -- what an image with three or
 * four grey classes needs and one level set cannot give.  A PAIR is two contexts A and B on one device with the same h, w and channel
 * count C: A holds phi1, B holds phi2.  The image is A's planes; B's planes are not read by the iteration (B must still hold an image:
 * its stop condition and its later mask calls are defined by it).  The pair has no object of its own and keeps nothing between calls;
 * every mask-based call (cvh_components, cvh_measure, cvh_contours*, cvh_score_mask*, cvh_morph_levelset, cvh_reinit, cvh_overlaps*)
 * works on either context unchanged.  The reference has no such model; the definition below IS the contract.
 *     H1 = H_eps(phi1), H2 = H_eps(phi2), f = I_k as double (H_eps, delta_eps, kappa exactly those of the two-phase step: the
 *     reference's regularized_heaviside, regularized_delta and curvature with its border rule)
 *     w11 = H1 H2, w10 = H1 (1 - H2), w01 = (1 - H1) H2, w00 = (1 - H1)(1 - H2);  c_ab[k] = sum f w_ab / sum w_ab over all pixels
 * One iteration updates both level sets from the OLD pair (Jacobi):
 *     F1 = sum_k [ H2 (-l1A[k] (f - c11[k])^2 + l2A[k] (f - c01[k])^2) + (1 - H2)(-l1A[k] (f - c10[k])^2 + l2A[k] (f - c00[k])^2) ]
 *     F2 = sum_k [ H1 (-l1B[k] (f - c11[k])^2 + l2B[k] (f - c10[k])^2) + (1 - H1)(-l1B[k] (f - c01[k])^2 + l2B[k] (f - c00[k])^2) ]
 *     d1 = dtA (muA kappa(phi1) - nuA + F1 / C) delta_eps(phi1),  phi1 <- phi1 + d1
 *     d2 = dtB (muB kappa(phi2) - nuB + F2 / C) delta_eps(phi2),  phi2 <- phi2 + d2
 * A's cvh_params govern phi1's equation (l1A = lambda1, l2A = lambda2 of A), B's govern phi2's; eps must be equal in both.  Per level
 * set this is the two-phase combine (src/main.cpp:985, folded as there: kappa (dt mu) + F (dt / C) - dt nu) with the region term
 * blended by the other level set's Heaviside.  The stop rule is tested after the update, as in the reference: the pair stops at the
 * first iteration with ||d1||_2 <= stop(A) and ||d2||_2 <= stop(B), stop(X) what cvh_get_stop_condition(X) returns; the stopping
 * iteration's update is kept, later iterations of the same call change nothing.  Arithmetic is A's "math_mode": CVH_MATH_STRICT the
 * op-by-op forms, CVH_MATH_FAST (the default) the forms and refinements of the wave kernels; both agree with a numpy restatement of
 * the definition to 1e-9 (tests/test_gpu_multiphase.py).
 * cvh_multiphase_run iterates until max_steps iterations are done (max_steps < 0: no bound) or the pair stops.  steps_done, norms
 * ({||d1||, ||d2||} of the last executed iteration) and trace may be NULL.  Row t of the trace (4 C + 2 doubles, at most trace_rows rows,
 * *rows written) is [c11[0..C), c10[..], c01[..], c00[..], ||d1||, ||d2||]: the means iteration t used and its two norms.  The call
 * settles both contexts as the getters do, takes the pair's initial sums itself, and ends with both contexts exactly as
 * cvh_set_levelset of the new doubles leaves them (a new run begins on each: counters 0, the two-phase means not yet taken); a
 * one-context run continued afterwards is bit for bit what it is after cvh_set_levelset of the fetched doubles.  Device work runs on
 * A's stream, joined with B's before and after; the host enqueues A's "sync_every" iterations at a time (two launches each) and waits
 * once per chunk for the pair's state.  Launches enqueued behind a stop return at once.  Workspaces (state block, partial sums,
 * trace) are A's, allocated on first use and kept; the level sets iterate in the contexts' own buffer pairs.  cvh_last_run_ms(A)
 * afterwards is the device's time from the first iteration's launch to the end of the last chunk (the waits between chunks included).
 * Determinism: every result depends on the inputs and the shape alone.  Partial sums are taken per ITEM of a fixed partition of the
 * plane (cvh_multiphase_geometry: strips of *strip_rows rows x *cols columns, *items of them; a function of h and w alone, not of the
 * device) and added in a fixed order by a one-workgroup launch; no atomics.  Two runs of the same pair give the same bits.  One call of
 * m + n iterations and two calls of m and of n give the same bits as well, in both arithmetic modes: the second call takes its initial
 * sums again, but over the same partition, in the same order and with the same form of H_eps per pixel (in CVH_MATH_FAST the form is
 * chosen per wave and row by the row's own pixels alone), of the very doubles the first call stored.
 * cvh_multiphase_means returns the 4 C means of the CURRENT pair, c[ab C + k] in the order 11, 10, 01, 00; it only reads.
 * cvh_multiphase_labels / _device write label = mask(A) + 2 mask(B) per pixel (0 .. 3), mask as cvh_get_mask(.., invert = 0) defines
 * it: one launch on A's stream; they only read.  The device form is ordered behind `stream` and in front of what is enqueued on it
 * later, and does not make the host wait.  A run of either context continued after a read-only call is bit-identical to one without it.
 * CVH_ERR_ARG: a NULL or identical pair, different devices, shapes or channel counts, different eps, "state" = 32 on either context,
 * h*w >= 2^28, a NULL output (c, labels, d_labels) or memory the device cannot address, a trace without rows or with trace_rows < 0.
 * CVH_ERR_STATE: a context without a level set, or (run, means) without an image.  Everything is checked before anything is touched;
 * the message is cvh_last_error(NULL)'s (and A's); after such a refusal the contexts are as they were and stay usable.  (A HIP error
 * inside a run -- CVH_ERR_HIP -- is another matter: the level sets may be partly iterated; give both contexts new level sets.)
 * Empty regions: there is no guard.  A region whose weight sum is exactly 0 has the means 0 / 0 = NaN, as IEEE division gives and as
 * cvh_get_means gives for a wholly empty side of one level set; a nearly empty region has whatever the quotient of its two sums is.
 * H_eps reaches 0 or 1 exactly only far from the front -- in CVH_MATH_FAST from |phi| of about 1e16 eps on, over the WHOLE plane.  The
 * NaN then reaches both level sets and both norms with the next iteration, the stop rule never fires on a NaN norm (the run ends at
 * max_steps), and none of it is an error.
 * cvh_multiphase_run_batch runs n pairs (as[i], bs[i]) in shared launches: steps_done[i], norms[2 i], norms[2 i + 1], traces[i] (NULL:
 * no trace for that pair; traces itself may be NULL) and rows[i] are pair i's, with cvh_multiphase_run's meaning; "the same context
 * twice" counts across as and bs.
 * A member is its own run: level set(s), steps_done[i], norm(s) and every trace row of member i are bit for bit what the single call
 * gives for that member alone from the same state -- in both "math_mode"s, for any n, any order of the members and any mix of shapes,
 * channel counts (1 and 3), radii, parameters and "math_mode"s -- and the member is left exactly as the single call leaves it.  (Both
 * kernels take their partial sums per item of a partition that depends on h and w alone and add them in a fixed order: a member's
 * bits cannot depend on who shares the launch.  The single call IS the batch of one member -- one host path; a call with one member hands its record to the kernels by value.)
 * Members stop independently: each keeps its own state block and stop flag, workgroups of a stopped member return at once, a stopped
 * member keeps its stopping iteration's update, and the call ends when every member has stopped or max_steps iterations are enqueued.
 * Launches: per iteration ONE launch per kernel and per (channel count, math mode) class present in the batch (the kernels are
 * templates on both); a finalise launch has one workgroup per member.  The member table -- one argument record per member with BOTH
 * buffers of every level set, blocks find their member through prefix block counts -- is uploaded once per call; an iteration's
 * parity travels as a kernel argument and nothing is uploaded between iterations.  The planes T_k / the initial sums are taken the
 * same way, once per call for all members.  The host waits ONCE per chunk of member 0's "sync_every" iterations, whatever n: every
 * finalise workgroup mirrors its member's state block in a contiguous state table, which comes down in one copy.
 * Work runs on member 0's stream (A0's for pairs), joined with every member's stream before and after.  Workspaces, traces and state
 * blocks stay the members' own; the table is member 0's, grown on demand and kept.  cvh_last_run_ms(member 0) is as for the single call.
 * Refusals: everything is checked before anything is touched, the message names the member index and is cvh_last_error(NULL)'s and
 * member 0's, and the contexts are as they were afterwards.  CVH_ERR_ARG: n <= 0, a NULL array or member, the same context twice
 * anywhere in the call, members on different devices, 2^31 or more workgroups in one launch, and every per-member refusal of the
 * single call; CVH_ERR_STATE as for the single call.  max_steps = 0 iterates nothing and returns zeros.
 * When it pays: measured once on an MI355X (tools/march_batch_probe.py, 64 iterations, us per pair-iteration, batch against a loop of
 * cvh_multiphase_run; one / three channels): 64 x 256^2 1.5 against 14.9 (9.7x) / 1.9 against 19.6 (10.5x); 32 x 512^2 3.8x / 3.9x; 8 x 1024^2 2.0x /
 * 2.1x; 2 x 2048^2 1.20x / 1.28x.  It lost at no shape measured.  A call with one pair launches the single call's by-value kernels.
 * Not here: the resident (LDS) flow, FP32 state, a four-phase energy, pyramids and reinitialisation inside the run (cvh_reinit on each
 * context between runs works), more than two level sets, batches across devices. */
int cvh_multiphase_run(cvh_context *a, cvh_context *b, int max_steps, int *steps_done, double *norms /* 2 */, double *trace, int trace_rows,
                       int *rows);
extern int cvh_multiphase_run_batch(cvh_context *const *as, cvh_context *const *bs, int n, int max_steps, int *steps_done /* n */, double *norms /* 2 n */,
                             double *const *traces /* n or NULL */, int trace_rows, int *rows /* n */);
int cvh_multiphase_means(cvh_context *a, cvh_context *b, double *c /* 4 C */);
int cvh_multiphase_labels(cvh_context *a, cvh_context *b, uint8_t *labels);   /* host bytes, 0 .. 3 */
int cvh_multiphase_labels_device(cvh_context *a, cvh_context *b, uint8_t *d_labels, void *stream);
void cvh_multiphase_geometry(int h, int w, int *cols, int *strip_rows, int *items);   /* pure host arithmetic; 0 rows / items: not a plane the calls take */

/* ---- Localised regions ----------------------------------------------------------------------------------------------------------
 * Localised (local region-based) Chan-Vese, after Lankton and Tannenbaum, Brox and Cremers, and Li's LBF: the two region means become
 * functions of the pixel, c1(p) and c2(p), taken over a window around p and retaken every iteration.  Every other flow of this library
 * fits each side of the contour with ONE mean per channel, which fails by construction under uneven illumination; this one changes the
 * model, not the image.  The reference has no such model; the definition below IS the contract.
 * Window: W(p) is the (2 R + 1)^2 square around p truncated at the plane's border -- exactly the window of "Local statistics" --
 * 1 <= R <= 127, n(p) = |W(p)|.
 * Weights are fixed-point: wq(p) = rint(H_eps(u(p)) 2^40) as an unsigned 64-bit integer in [0, 2^40], H_eps the two-phase step's
 * (regularized_heaviside) in the context's "math_mode"; the outside weight is the exact complement 2^40 - wq(p).  wq(p) is a function
 * of the stored double u(p) alone.
 * Sums are exact integers, f_k = I_k as an integer:
 *     A(p) = sum_{q in W(p)} wq(q)      S_k(p) = sum_W wq(q) f_k(q)      T_k(p) = sum_W f_k(q)
 *     B(p) = n(p) 2^40 - A(p)           S'_k(p) = T_k(p) 2^40 - S_k(p)
 * all below 2^64 (65025 * 255 * 2^40 < 2^64: a static_assert in the library); n and T_k do not depend on u and are taken once per call.
 * Means: c1_k(p) = (double)S_k(p) / (double)A(p), c2_k(p) = (double)S'_k(p) / (double)B(p): each conversion rounds to nearest, then
 * one IEEE division.  There is no guard: A = 0 or B = 0 gives 0 / 0 = NaN, as the other flows give for an empty side.  wq reaches 0
 * or 2^40 from |u| of about 2^41 eps / pi (7e11 eps) on, so that needs a whole window that far on one side of the front.
 * Update (Jacobi: every window sum of iteration t is taken from the u that iteration t reads):
 *     F(p) = sum_k [ -lambda1[k] (f_k - c1_k(p))^2 + lambda2[k] (f_k - c2_k(p))^2 ]
 *     d = dt (mu kappa(u) - nu + F / C) delta_eps(u), folded exactly as the two-phase combine (kappa (dt mu) + F (dt / C) - dt nu);  u <- u + d
 * kappa, delta_eps, the border rule, the stop rule (||d||_2 <= cvh_get_stop_condition, tested after the update) and the kept stopping
 * iteration are as in "Four phases".  Arithmetic is the context's "math_mode": CVH_MATH_STRICT the op-by-op forms, CVH_MATH_FAST (the
 * default) the wave kernels' forms of H_eps and delta_eps -- the form of H_eps chosen per pixel by the pixel's own stored value.  Both
 * agree with a numpy restatement of this definition within a bound derived from perturbing H_eps by 2 ulp (tests/localized_util.py).
 * The local force is small: far from the front both local means tend to the window mean and F is noise.  Start near the object (Otsu,
 * rect, disk, mask: "Initial level sets") and raise mu (of the order of 100 for 8-bit images with the default lambdas).
 * cvh_localized_run iterates until max_steps iterations are done (max_steps < 0: no bound) or the stop rule fires.  steps_done, norm
 * (||d|| of the last executed iteration) and trace may be NULL; row t of the trace is ONE double, iteration t's ||d|| (at most
 * trace_rows rows, *rows written).  The call settles the context as the getters do and ends with it exactly as cvh_set_levelset of
 * the new doubles leaves it (a new run begins: counters 0, the two-phase means not yet taken); a two-phase run continued afterwards is
 * bit for bit what it is after cvh_set_levelset of the fetched doubles.  The host enqueues "sync_every" iterations at a time (three
 * launches each: row pass, step, finalise) and waits once per chunk for the state block; launches enqueued behind a stop return at
 * once.  The workspace (state block, partial sums, 1 + C planes of horizontal window sums, C planes of T_k: 8 + 12 C bytes per pixel,
 * whatever R) and the trace are the context's, allocated on first use and kept.  cvh_last_run_ms afterwards is the device's time from
 * the first iteration's launch to the end of the last chunk.
 * Determinism: the window sums are integers -- the same bits in any order and for any neighbour in the plane.  ||d||^2 is summed per
 * ITEM of a fixed partition (cvh_localized_geometry: *items items of *item_rows rows x *cols columns, a function of h and w alone) and
 * the items are added in index order by a one-workgroup launch; no atomics.  *strip_rows, the rows one wave marches down, is a whole
 * number of items chosen from R (at least 2 (2 R + 1) rows: a strip's lead-in of 2 R + 1 workspace rows is at most a third of what it
 * reads) and has no bearing on any result.  Two runs give the same bits; m + n iterations in one call equal m then n in two calls bit
 * for bit, in both arithmetic modes.
 * cvh_localized_means returns, for the CURRENT level set, the host planes c1, c2 (C h w doubles, plane k first), wq and a (h w) and
 * s (C h w): the bias-field picture.  Any may be NULL, not all.  It only reads: a run continued after it is bit-identical to one
 * without it.  The planes are staged on the device for the length of the call.
 * CVH_ERR_ARG: R outside 1 .. 127, "state" = 32, h*w >= 2^28, every output NULL, a trace without rows or with trace_rows < 0.
 * CVH_ERR_STATE: no image or no level set.  Everything is checked before anything is touched; the message is cvh_last_error's; after
 * such a refusal the context is as it was and stays usable.
 * cvh_localized_run_batch runs n contexts in shared launches, member i with radius[i]: steps_done[i], norms[i], traces[i] (NULL: no
 * trace for that member; traces itself may be NULL) and rows[i] are member i's, with cvh_localized_run's meaning.
 * A member is its own run: level set(s), steps_done[i], norm(s) and every trace row of member i are bit for bit what the single call
 * gives for that member alone from the same state -- in both "math_mode"s, for any n, any order of the members and any mix of shapes,
 * channel counts (1 and 3), radii, parameters and "math_mode"s -- and the member is left exactly as the single call leaves it.  (Both
 * kernels take their partial sums per item of a partition that depends on h and w alone and add them in a fixed order: a member's
 * bits cannot depend on who shares the launch.  The single call IS the batch of one member -- one host path; a call with one member hands its record to the kernels by value.)
 * Members stop independently: each keeps its own state block and stop flag, workgroups of a stopped member return at once, a stopped
 * member keeps its stopping iteration's update, and the call ends when every member has stopped or max_steps iterations are enqueued.
 * Launches: per iteration ONE launch per kernel and per (channel count, math mode) class present in the batch (the kernels are
 * templates on both); a finalise launch has one workgroup per member.  The member table -- one argument record per member with BOTH
 * buffers of every level set, blocks find their member through prefix block counts -- is uploaded once per call; an iteration's
 * parity travels as a kernel argument and nothing is uploaded between iterations.  The planes T_k / the initial sums are taken the
 * same way, once per call for all members.  The host waits ONCE per chunk of member 0's "sync_every" iterations, whatever n: every
 * finalise workgroup mirrors its member's state block in a contiguous state table, which comes down in one copy.
 * Work runs on member 0's stream (A0's for pairs), joined with every member's stream before and after.  Workspaces, traces and state
 * blocks stay the members' own; the table is member 0's, grown on demand and kept.  cvh_last_run_ms(member 0) is as for the single call.
 * Refusals: everything is checked before anything is touched, the message names the member index and is cvh_last_error(NULL)'s and
 * member 0's, and the contexts are as they were afterwards.  CVH_ERR_ARG: n <= 0, a NULL array or member, the same context twice
 * anywhere in the call, members on different devices, 2^31 or more workgroups in one launch, and every per-member refusal of the
 * single call; CVH_ERR_STATE as for the single call.  max_steps = 0 iterates nothing and returns zeros.
 * When it pays: measured once on an MI355X (tools/march_batch_probe.py, 64 iterations, us per member-iteration, batch against a loop of
 * cvh_localized_run): 64 x 256^2 2.1 against 25.3 at R = 2 (11.9x) and 2.4 against 53.7 at R = 10 (22.7x), three channels 7.9x / 16.5x; 32 x 512^2
 * 5.2x / 9.7x (three channels 3.6x / 6.5x); 8 x 1024^2 2.1x / 3.6x (1.6x / 2.4x); 2 x 2048^2 1.08x / 1.24x, and with three channels NOTHING (0.99x /
 * 1.01x: one member fills the card).  A call with one member launches the single call's by-value kernels.
 * Not here: the resident (LDS) flow, FP32 state, a localised energy, four phases with local means, pyramids or reinitialisation inside
 * the run, Gaussian windows, a global / local blend, batches across devices. */
int cvh_localized_run(cvh_context *ctx, int radius, int max_steps, int *steps_done, double *norm, double *trace, int trace_rows, int *rows);
extern int cvh_localized_run_batch(cvh_context *const *ctxs, int n, const int *radius /* n */, int max_steps, int *steps_done /* n */, double *norms /* n */,
                            double *const *traces /* n or NULL */, int trace_rows, int *rows /* n */);
int cvh_localized_means(cvh_context *ctx, int radius, double *c1, double *c2, uint64_t *wq, uint64_t *a, uint64_t *s);
void cvh_localized_geometry(int h, int w, int radius, int *cols, int *item_rows, int *items, int *strip_rows);   /* pure host arithmetic; 0 rows / items: not a plane or radius the calls take */

/* ---- Edge-weighted length ---------------------------------------------------------------------------------------------------------
 * Geodesic (edge-weighted) Chan-Vese, after Caselles, Kimmel and Sapiro and Bresson et al.: the length term mu int |grad H(u)| of every
 * other flow of this library becomes mu int g |grad H(u)| with an edge-stopping weight g, about 1 in flat areas and near 0 on image
 * edges: the contour is smoothed hard where nothing happens and left alone where the image says "boundary".  One level set, global
 * means.  The reference has no such model; the definitions below ARE the contract.
 * The EDGE PLANE gq of a context: h w uint16_t, row-major, values 0 .. 32768, g = gq 2^-15 exactly (g = 1 is representable; the step
 * reads 2 bytes per pixel).  It is allocated by the first call that writes it and kept until replaced.  cvh_set_image*, the calls that
 * write planes (Perona-Malik, colour, local, rank, restrict) and the level-set calls do NOT touch it: after the planes change, build it again.
 * cvh_set_edge_map / cvh_get_edge_map move it from / to host memory; a value above 32768 is CVH_ERR_ARG, checked on the host before
 * anything is touched.  cvh_set_edge_map_device / cvh_get_edge_map_device take device memory (2-byte aligned) and a stream: ordered
 * behind `stream` and in front of what is enqueued on it later by events, as the other _device calls, and they do not make the host
 * wait; there the range check is a device-side CLAMP to 32768.
 * cvh_edge_map(dst, src, K) builds dst's edge plane from the planes of src as they are now; src may be dst, must have dst's h and w and
 * device, and is only read; C below is src's channel count.  cvh_edge_map_batch does n pairs of any mix of shapes and channel counts
 * in one launch; a destination may be listed once, sources freely.  Integer and IEEE, so that every value is defined exactly:
 *     f_k = plane k as an integer, coordinates clamped to the plane (replicate border)
 *     sx_k, sy_k = the 3 x 3 Sobel sums (weights 1, 2, 1; differences of the columns / rows +-1) as int32
 *     m2 = sum_k (sx_k^2 + sy_k^2)                      (at most 3 * 2 * 1020^2)
 *     den = ((64.0 * C) * K) * K, taken once on the host   (64: Sobel sums -> unit-spacing gradient; C: the mean over channels, as F / C)
 *     gq = (uint16) rint(32768.0 / (1.0 + (double)m2 / den))   -- one conversion, a division, an addition, a division, round-half-even
 * This is the edge-stopping function 1 / (1 + |grad I|^2 / K^2) of cvh_perona_malik.  CVH_ERR_ARG: K not finite, K <= 0, den not finite,
 * NULL or differently shaped pairs, different devices; CVH_ERR_STATE: a source without an image.  Smoothing before the gradient is the
 * caller's, with calls that exist: run cvh_perona_malik on the context first, or build the map from a second context that holds
 * cvh_local_planes' mean.  There is no Gaussian in these calls themselves: for the textbook G_sigma * I, build the map from a
 * context that holds the BLUR planes of cvh_smooth_planes ("Smoothing").
 * The iteration, with nx, ny, H_eps, delta_eps and the border rule exactly those of the two-phase step:
 *     Gx(p) = g(p) nx(p)      Gy(p) = g(p) ny(p)                                      (one rounding each)
 *     kappa_g(r, c) = (c > 0 ? Gx(r, c) - Gx(r, c-1) : 0) + (r > 0 ? Gy(r, c) - Gy(r-1, c) : 0)
 *     c1[k] = sum f_k H / sum H      c2[k] = sum f_k (1 - H) / sum (1 - H)   over all pixels, no guard (0 / 0 = NaN, as elsewhere);
 *             the outside sums are taken as complements, (sum f_k - sum f_k H) / (h w - sum H): sum f_k is an exact integer
 *     F = sum_k [ -lambda1[k] (f_k - c1[k])^2 + lambda2[k] (f_k - c2[k])^2 ]
 *     d = dt (mu kappa_g - nu + F / C) delta_eps(u), folded as the two-phase combine;   u <- u + d
 * With gq = 32768 everywhere this is the two-phase model.  Everything else reads as in "Four phases": Jacobi iteration; the stop rule
 * ||d||_2 <= cvh_get_stop_condition tested after the update, the stopping iteration kept, later launches returning at once;
 * "math_mode" STRICT and FAST (the form of H_eps chosen per wave and row by the row's own pixels); both agree with a numpy restatement
 * to 1e-9 (tests/test_gpu_geodesic.py).  cvh_geodesic_run iterates until max_steps iterations are done (< 0: no bound) or the stop rule
 * fires; steps_done, norm and trace may be NULL; row t of the trace (2 C + 1 doubles, at most trace_rows rows, *rows written) is
 * [c1[0..C), c2[0..C), ||d||]: the means iteration t used and its norm.  The call settles the context, takes the initial sums itself
 * and leaves the context exactly as cvh_set_levelset of the new doubles leaves it; a two-phase run continued afterwards is bit for bit
 * what it is after cvh_set_levelset of the fetched doubles.  The edge plane is only read.  The host enqueues "sync_every" iterations at
 * a time (two launches each) and waits once per chunk; cvh_last_run_ms is as for "Four phases".
 * Determinism: partial sums per ITEM of the four-phase partition (cvh_geodesic_geometry: strips of *strip_rows rows x *cols columns,
 * *items of them, a function of h and w alone) added in a fixed order by a one-workgroup launch; no atomics.  Two runs give the same
 * bits; m + n iterations in one call equal m then n in two calls bit for bit, in both modes.
 * cvh_geodesic_run_batch runs n contexts in shared launches with the meaning, the guarantees (a member is bit for bit its own single
 * run, for any mix of shapes, channel counts, parameters and modes, in any order), the launches and the refusals of
 * cvh_localized_run_batch; a batch of one launches the single call's by-value kernels.
 * CVH_ERR_STATE: no image, no level set or no edge plane.  CVH_ERR_ARG: "state" = 32, h*w >= 2^28, a trace without rows or with
 * trace_rows < 0, and for the batch n <= 0, a NULL array or member, the same context twice, different devices, 2^31 workgroups.
 * Everything is checked before anything is touched; after a refusal the contexts are as they were.
 * Not here: an edge-weighted energy (cvh_energy does not know g: it reports the unweighted functional), the resident flow, FP32 state,
 * edge weighting inside four-phase or localised runs, pyramids or reinitialisation inside the run, a g-weighted balloon term. */
int cvh_set_edge_map(cvh_context *ctx, const uint16_t *gq);   /* host, h w values */
int cvh_get_edge_map(cvh_context *ctx, uint16_t *gq);
int cvh_set_edge_map_device(cvh_context *ctx, const uint16_t *d_gq, void *stream);
int cvh_get_edge_map_device(cvh_context *ctx, uint16_t *d_gq, void *stream);
int cvh_edge_map(cvh_context *dst, cvh_context *src, double K);
int cvh_edge_map_batch(cvh_context *const *dsts, cvh_context *const *srcs, int n, const double *K /* n */);
int cvh_geodesic_run(cvh_context *ctx, int max_steps, int *steps_done, double *norm, double *trace, int trace_rows, int *rows);
int cvh_geodesic_run_batch(cvh_context *const *ctxs, int n, int max_steps, int *steps_done /* n */, double *norms /* n */,
                           double *const *traces /* n or NULL */, int trace_rows, int *rows /* n */);
void cvh_geodesic_geometry(int h, int w, int *cols, int *strip_rows, int *items);   /* pure host arithmetic; 0 rows / items: not a plane the calls take */

/* ---- Convex relaxation -------------------------------------------------------------------------------------------------------------
 * The convex relaxation of two-phase Chan-Vese (Chan, Esedoglu and Nikolova), solved by the primal-dual iteration of Chambolle and
 * Pock; with an edge plane it is the weighted model of Bresson et al.  Every other flow of this library descends on a level set and
 * ends in a minimum that depends on the start.  Here, for fixed means, a function v with 0 <= v <= 1 takes the place of H(u), the
 * problem in v is convex, and any threshold of a minimiser is a global minimiser of the two-phase functional: no eps, no delta
 * function, no reinitialisation.  The reference has no such model; the definitions below ARE the contract.
 * STATE.  A context gets a relaxation state in a workspace it owns, allocated by the first call and kept: v, the extrapolated vbar and
 * the dual field q = (qx, qy), h w doubles each, row-major; vbar, qx and qy are double-buffered (a wave recomputes halo values from the
 * old ones), v is updated in place: 7 planes, 56 bytes per pixel.  No other call reads or clears it.
 * START (resume = 0): v0 = 1 where (float)u > 0, else 0 -- the bytes of cvh_get_mask with invert = 0 --, vbar0 = v0, q = 0.  The sums of
 * v0 and of f_k v0 are exact integers in any order, so the first means are bit-defined.
 * ONE ITERATION, everything taken from the old v, vbar and q (Jacobi); f_k = plane k, tau and sigma the call's, mu, nu, lambda1[k],
 * lambda2[k] the context's as they are now (dt and eps are not read), C the channel count.  In STRICT mode the operation order is
 * exactly this, one rounding per operation and no contraction:
 *     a_k = f_k - c1[k];  b_k = f_k - c2[k];  t_k = lambda1[k] (a_k a_k) - lambda2[k] (b_k b_k)
 *     r   = nu + ((t_0 + t_1) + t_2) / C                                  (C = 1: nu + t_0)
 *     dx  = c < w-1 ? vbar(r, c+1) - vbar(r, c) : 0;   dy = r < h-1 ? vbar(r+1, c) - vbar(r, c) : 0
 *     tx  = qx + sigma dx;  ty = qy + sigma dy;  s = sqrt(tx tx + ty ty);  rho = mu g        (g = gq 2^-15, or 1 with use_edge = 0)
 *     s > rho ?  k = rho / s, qx' = tx k, qy' = ty k   :   qx' = tx, qy' = ty
 *     div = (qx' - (c > 0 ? qx'(r, c-1) : 0)) + (qy' - (r > 0 ? qy'(r-1, c) : 0))
 *     x   = v + tau (div - r);   v' = x < 0 ? 0 : (x > 1 ? 1 : x)                          (a NaN stays a NaN: no guard, as elsewhere)
 *     vbar' = (v' + v') - v;     d = v' - v
 * MEANS.  c1[k] = sum f_k v / sum v, c2[k] = (sum f_k - sum f_k v) / (h w - sum v), the complement as the geodesic flow takes it, no
 * guard.  They are taken at the start and retaken after every means_every-th iteration (means_every = 0: never after the start); the
 * count since the last retake belongs to the state and goes on across resumed calls.  Row t of the trace (2 C + 1 doubles, at most
 * trace_rows rows, *rows written) is [c1[0..C), c2[0..C), ||d||_2]: the means iteration t used and its norm.
 * STOP.  The run stops after the iteration with ||d||_2 <= stop_rms sqrt(h w), the product taken once on the host; stop_rms < 0: no
 * rule; stop_rms = 0 stops at an exact fixed point alone (the noisy disk of tests/convex_util.py reaches one in 5 iterations, every v in {0, 1}; the
 * harder demonstration scenes were run with stop_rms = 1e-5).  The stopping iteration is kept,
 * later launches return at once.  cvh_get_stop_condition is in grey-level units and is not used here.  max_steps < 0: no bound.
 * RESUME (resume = 1) continues the stored v, vbar, q, the means and the count since the last retake with the planes and parameters as
 * they are now, and does not read the level set: m + n iterations in one call equal m then n (resumed) bit for bit, in both math modes
 * and for any means_every.
 * END of every call: the level set becomes u = v - 0.5, one rounding per pixel, and the context is left exactly as cvh_set_levelset of
 * those doubles leaves it: the mask calls, components, contours, scores, cvh_reinit and further level-set iterations see the
 * thresholded result; a two-phase run continued afterwards is bit for bit what it is after cvh_set_levelset of the fetched doubles.
 * "math_mode": STRICT follows the lines above -- with means_every = 0 every value is bit-defined, and v, qx, qy equal a numpy
 * restatement (tests/convex_util.py) bit for bit; FAST uses fused multiply-adds and the refined reciprocal square root in the
 * projection (taken where tx tx + ty ty > rho rho).  Otherwise both agree with the restatement to 1e-9.
 * Determinism: partial sums per ITEM of the four-phase partition (cvh_convex_geometry: strips of *strip_rows rows x *cols columns,
 * *items of them, a function of h and w alone) added in a fixed order by a one-workgroup launch; no atomics.  Two runs give the same
 * bits.  The host enqueues "sync_every" iterations at a time (two launches each) and waits once per chunk.
 * cvh_convex_run_batch runs n contexts, member i with params[i], in shared launches with the meaning, the guarantees (a member is bit
 * for bit its own single run, for any mix of shapes, channel counts, parameters and modes, in any order; members stop on their own),
 * the launches and the refusals of cvh_geodesic_run_batch; a batch of one launches the single call's by-value kernels.
 * cvh_get_relaxed copies v and the current qx, qy to host memory (any pointer may be NULL); cvh_get_relaxed_device copies v to device
 * memory (8-byte aligned), ordered against `stream` by events as the other _device calls, without a host wait.
 * CVH_ERR_ARG: NULL params; tau or sigma not finite or <= 0; 8 tau sigma > 1 (the step-size bound of the forward-difference gradient);
 * a NaN stop_rms; means_every < 0; "state" = 32; h*w >= 2^28; a trace without rows or with trace_rows < 0; and for the batch what
 * cvh_geodesic_run_batch refuses.  CVH_ERR_STATE: no image; no level set with resume = 0; no relaxation state with resume = 1, or in
 * cvh_get_relaxed*; no edge plane with use_edge = 1.  Everything is checked before anything is touched; after a refusal the contexts
 * are as they were.
 * Not here: the primal-dual gap or a relaxed energy, FP32 dual state, the resident flow, four-phase or localised convex models,
 * pyramids inside the run. */
typedef struct cvh_convex_params {
  double tau, sigma;                /* primal and dual step: finite, > 0, 8 tau sigma <= 1 */
  double stop_rms;                  /* stop at ||d||_2 <= stop_rms sqrt(h w); < 0: no rule */
  int means_every;                  /* retake the means after every means_every-th iteration; 0: never after the start */
  int use_edge;                     /* 1: rho = mu g with the context's edge plane */
  int resume;                       /* 1: continue the stored relaxation state */
} cvh_convex_params;
int cvh_convex_run(cvh_context *ctx, int max_steps, const cvh_convex_params *params, int *steps_done, double *norm, double *trace, int trace_rows,
                   int *rows);
int cvh_convex_run_batch(cvh_context *const *ctxs, int n, int max_steps, const cvh_convex_params *params /* n */, int *steps_done /* n */,
                         double *norms /* n */, double *const *traces /* n or NULL */, int trace_rows, int *rows /* n */);
int cvh_get_relaxed(cvh_context *ctx, double *v, double *qx, double *qy);   /* host, h w doubles each; any may be NULL */
int cvh_get_relaxed_device(cvh_context *ctx, double *d_v, void *stream);
void cvh_convex_geometry(int h, int w, int *cols, int *strip_rows, int *items);   /* pure host arithmetic; 0 rows / items: not a plane the calls take */

/* Library version string, e.g. "chanvese_hip 0.1 (gfx950)". */
const char *cvh_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CHANVESE_HIP_H */
