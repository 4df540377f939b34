// csv_run.hip — the CSV steps of one context: launch geometry and arguments, strip tables, the per-launch, graph and resident flows,
// chain flush and sync (cvh_enqueue_steps, cvh_warm, cvh_sync, cvh_run).
#include "cvh_host.h"

// Which step kernel runs and on what grid (g.strip: 0 tile kernel, 2 wave kernel, 3 wave kernel with 2 pixels per lane).
Geometry resolve_geometry(const cvh_context *c)
{
  Geometry g;
  g.strip = 0;
  const int cus = c->geom_cus > 0 ? c->geom_cus : c->num_cus;   // what the automatic strip count fills (a fused batch: a share)
  // default: the wave kernel (any width; fastest measured); it addresses the level set through
  // buffer instructions with 32-bit byte offsets and marks dropped lanes with offset 2^31, so
  // images of 2^28 pixels (2 GiB of level set) or more use the tile kernel
  // auto: the 2-pixel kernel from 0.6 Mpixel up (end of round 2, one context per size, 2-pixel with its cache policy chosen by
  // footprint vs 1-pixel: 3000x4000 40.3 vs 43.8 us, 4096^2 59.4 vs 64.7, 4608^2 80.5 vs 87.2, 5120^2 93.1 vs 97.2, 6144^2 133.0 vs
  // 140.7, 4320x7680 122.7 vs 123.2, 8192^2 243.3 vs 245.5)
  // three channels: the 2-pixel flavour exists in FAST arithmetic only; with equal strips (no class skew) it is the faster one from
  // round 3 on (4096^2 x 3, one context, alternating: 73.3 vs 74.9 us; bench lines of one session: 72.9 / 74.3 vs 74.5 / 76.1 us)
  const bool two_px_c3 = c->C == 3 && use_fast(c) && (c->kernel == 3 || c->kernel == -1 || c->state_bits == 32);
  if ((c->kernel == 3 || c->state_bits == 32 || (c->kernel == -1 && c->n >= (size_t)600000)) && (c->C == 1 || two_px_c3) && c->w % 16 == 0 &&
      c->w >= 144 && c->n < ((size_t)1 << 28)) {
    // wave kernel with 2 pixels per lane: 126 output columns per wave; workgroup = 2 wave-columns x 2 strips;
    // one round of resident waves (3 or 4 per SIMD)
    g.strip = 3;
    g.rows = 4;
    g.tiles_x = (c->w + cvh_wave2_cols() - 1) / cvh_wave2_cols();
    const int nbc = (g.tiles_x + 1) / 2;
    int sr = c->strip_rows, small_exact = 0;
    if (sr <= 0) {
      const int occ = use_fast(c) ? (c->wave_minw == 4 ? 4 : 3) : 2;   // as compiled: cvh_launch_wave2
      int nstrips = 2 * ((cus * occ) / nbc);
      // small planes (a full round would mean strips of < 13 rows: 3 halo rows and a pipeline fill each): ~1.8 workgroups
      // per CU instead -- measured at 2048^2: 16 rows 23.2, 18 rows 24.1, 20 rows 21.4, 22 rows 22.7, 24 rows 22.8 us
      // (round 3, exact strip counts at 2048^2, one context: 56 strips 22.8 us, 84 21.2, 100 21.1, 104 20.8, 108 21.2, 112 20.7, 114 22.1 --
      // one workgroup more than two per CU --, 128 21.4, 140 21.1, 168 21.6: flat from 84 to 168 except just above a multiple of the CU
      // count; TWO workgroups per CU, never more)
      bool exact = false;
      if (nstrips > 160) { nstrips = 2 * ((2 * cus) / nbc); if (nstrips < 2) nstrips = 2; exact = true; }
      if (nstrips < 1) nstrips = 1;
      sr = (c->h + nstrips - 1) / nstrips;
      if (sr < 8) { sr = 8; exact = false; }
      if (exact && c->wave_cls && c->wave_xcd) small_exact = nstrips;   // the class-major table deals rows by weight: any count works
    }
    g.strip_rows = sr;
    g.tiles_y = small_exact ? small_exact : (c->h + sr - 1) / sr;
    if (c->strips > 0 && c->strip_rows <= 0 && c->wave_cls && c->wave_xcd) {   // exact count ("strips"): the class-major table deals rows by weight
      g.tiles_y = c->strips;
      g.strip_rows = (c->h + c->strips - 1) / c->strips;
      if (g.strip_rows < 8) { g.strip_rows = 8; g.tiles_y = (c->h + 7) / 8; }
    }
    g.nblocks = nbc * ((g.tiles_y + 1) / 2);
    return g;
  }
  if ((c->kernel == 2 || c->kernel == 3 || c->kernel == -1) && c->n < ((size_t)1 << 28)) {
    // wave kernel: 63 output columns per wave, strip_rows rows per wave, 4 waves per workgroup;
    // one round of resident waves (wave_minw per SIMD)
    g.strip = 2;
    g.rows = 4;
    g.tiles_x = (c->w + cvh_wave_cols() - 1) / cvh_wave_cols();
    int sr = c->strip_rows;
    if (sr <= 0) {
      // waves per SIMD the kernel flavour is compiled for (csv_wave_kernel.hip, launch_wave_c)
      const int occ = use_fast(c) ? (c->C == 3 ? 3 : c->wave_minw) : (c->C == 3 ? 2 : 3);
      int nstrips = (cus * occ) / ((g.tiles_x + 3) / 4);
      // Every strip re-reads 3 halo rows and fills its pipeline once: measured on MI355X (512^2 ..
      // 4096^2, tools/size_sweep.sh) a full round of resident waves is best at 4096^2 (75 strips) and
      // 64 strips wherever residency would allow many more (smaller images).
      if (nstrips > 80) nstrips = 64;
      if (nstrips < 1) nstrips = 1;
      sr = (c->h + nstrips - 1) / nstrips;
      if (sr < 8) sr = 8;  // shorter strips only pay prologue overhead
    }
    g.strip_rows = sr;
    g.tiles_y = (c->h + sr - 1) / sr;
    g.nblocks = ((g.tiles_x + 3) / 4) * g.tiles_y;  // 4 adjacent wave-columns per workgroup
    return g;
  }
  g.rows = c->tile_rows == 16 ? 16 : 14;  // auto = 14: keeps 4 workgroups per CU beside the tables
  cvh_step_grid(c->h, c->w, g.rows, &g.tiles_x, &g.tiles_y);
  g.strip_rows = g.rows;
  g.nblocks = g.tiles_x * g.tiles_y;
  return g;
}

bool use_chain(const cvh_context *c, const Geometry &g)
{
  return (g.strip == 3 || g.strip == 2) && use_fast(c) && c->finalize_mode == 0 && c->chain_opt;
}

// ---- One-buffer flow of the 2-pixel kernel (csv_wave2_ob_kernel, csv_wave2_kernel.hip; layout: cvh_internal.h, cvh_ob_*).  The ping-pong pair of a 4096^2 plane
// (285 MB with the image) does not fit the 256 MiB Infinity Cache, one padded buffer (160 MB) does.  The flow exists for one channel, FAST
// arithmetic, the FP64 state and a context's own per-launch launches.  It is taken only where the run cannot stop (tol == 0): in chain
// mode the launch behind a stop has already computed one more iteration when the bookkeeper fires the rule, which the pair survives (the
// stopped level set is the buffer that launch read) and one buffer would not -- every run with tol > 0 keeps the pair.  (A tol = 0 run
// stops only on a norm of exactly 0, where the iteration beside the stop rewrites every cell with the value it holds.)
bool one_buffer_rule(const cvh_context *c, const Geometry &g, bool alone)
{
  if (c->one_buffer == 0 || g.strip != 3 || c->C != 1 || !use_fast(c) || c->state_bits != 64 || c->p.tol != 0.0) return false;
  if (c->wave_pol == 2 || c->in_batch) return false;   // the diagnostic load policy; a fused batch's member
  if (c->resident_opt != 0) {   // planes the resident flow may take stay its
    ResidentGeom rg;
    if (resident_tile_grid(c->h, c->w, c->C, c->num_cus, c->num_cus, &rg)) return false;
  }
  const double slab = (double)cvh_ob_rows(c->h, g.tiles_y) * cvh_ob_pitch(c->w, g.tiles_x) * sizeof(double);
  if (slab >= 2147483648.0) return false;   // 32-bit byte offsets, dropped lanes at 2^31
  if (c->one_buffer == 1) return true;
  // auto: a single live context whose pair exceeds what the cache holds reliably while one buffer (pads, shadow rows, image) stays below it
  // -- in the automatic geometry, where the flow was measured against the pair; a caller who chose the kernel or tuned
  // its strips keeps the flow that choice was made for (as the resident flow's automatic rule steps aside, resident_geometry)
  if (c->kernel != -1 || c->strip_rows != 0 || c->strips != 0 || c->wave_cls != 1 || c->wave_cskew != 500 || c->wave_skew != 0) return false;
  return alone && (double)c->n * 17.0 > kCachedFootprint && slab + (double)c->n <= kCachedFootprint;
}

bool wants_one_buffer(const cvh_context *c, const Geometry &g) { return one_buffer_rule(c, g, run_is_alone(c)); }

// The strips' shadow-row table (CVH_OB_TAB ints per strip, cvh_internal.h) from the strip table b[0 .. S]: a strip reads rows
// max(s0 - 2, 0), s0 - 1 and s1 of its neighbours through its three shadow rows; each of those rows is written there by the strip that owns
// it.  Strips without rows own nothing and need nothing.
void one_buffer_table(const std::vector<int> &b, int h, std::vector<int> &tab)
{
  const int S = (int)b.size() - 1;
  tab.assign((size_t)S * CVH_OB_TAB, -1);
  std::vector<int> ne;
  for (int k = 0; k < S; ++k) if (b[k + 1] > b[k]) ne.push_back(k);
  for (size_t t = 0; t < ne.size(); ++t) {
    const int k = ne[t], kp = t > 0 ? ne[t - 1] : -1, kn = t + 1 < ne.size() ? ne[t + 1] : -1, knn = t + 2 < ne.size() ? ne[t + 2] : -1;
    const int s0 = b[k], s1 = b[k + 1];
    int *T = &tab[(size_t)k * CVH_OB_TAB];
    if (kp >= 0) T[0] = 3 * kp + 2;                          // first row: row s1 of the strip above
    if (kn >= 0) {
      T[1] = 3 * kn + 1;                                     // last row: row s0 - 1 of the strip below
      if (s1 - s0 >= 2) T[3] = 3 * kn;                       // last row but one: its row s0 - 2
      else if (s0 == 0) T[2] = 3 * kn;                       // (a one-row strip at the top: max(s0 - 2, 0) of the strip below is that row)
    }
    if (knn >= 0 && b[kn + 1] - b[kn] == 1) T[4] = 3 * knn;  // last row: row s0 - 2 of the strip behind a one-row strip
    if (s0 > 0) { T[5] = s0 >= 2 ? s0 - 2 : 0; T[6] = s0 - 1; }
    if (s1 < h) T[7] = s1;
  }
}

// Called where a context's own per-launch launches are about to be enqueued, behind upload_strip_bounds: enters the one-buffer flow (the
// slab takes the level set over from d_u[], with the pads and shadow rows of the parity the next launch reads), keeps it, or leaves it.
int one_buffer_flow(cvh_context *c, const Geometry &g)
{
  if (!wants_one_buffer(c, g)) return one_buffer_leave(c);
  const int pitch = cvh_ob_pitch(c->w, g.tiles_x), rows = cvh_ob_rows(c->h, g.tiles_y);
  const int key[6] = {c->bounds_key[0], c->bounds_key[1], c->bounds_key[2], c->bounds_key[3], pitch, rows};
  if (c->ob_live && !memcmp(key, c->ob_key, sizeof(key))) return CVH_OK;
  int rc = c->ob_live ? one_buffer_leave(c) : settle(c);     // (another strip table: through the mirror)
  if (rc == CVH_OK) rc = ensure_f64_mirror(c);
  if (rc != CVH_OK) return rc;
  const size_t bytes = (size_t)rows * pitch * sizeof(double);
  if (bytes > c->ob_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->d_ob) { HIPCHK(c, hipFree(c->d_ob)); c->d_ob = nullptr; c->ob_cap = 0; }
    HIPCHK(c, hipMalloc((void **)&c->d_ob, bytes));
    c->ob_cap = bytes;
  }
  // (cleared: the pads of the shadow rows are never written, and a lane that owns no pixel computes with what it reads there)
  HIPCHK(c, hipMemsetAsync(c->d_ob, 0, bytes, c->stream));
  if (!c->d_ob_tab) HIPCHK(c, hipMalloc((void **)&c->d_ob_tab, (size_t)(c->h + 1) * CVH_OB_TAB * sizeof(int)));
  std::vector<int> tab;
  one_buffer_table(c->h_bounds, c->h, tab);
  if ((int)tab.size() != g.tiles_y * CVH_OB_TAB) return fail(c, CVH_ERR_STATE, "one-buffer flow: the strip table does not match the geometry");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->d_ob_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
  const int par = (c->cur_base + c->enqueued) & 1;
  HIPCHK(c, cvh_launch_ob_pack(c->d_u[par], c->d_ob, c->d_ob_tab, c->h, c->w, g.tiles_x, g.tiles_y, par, c->stream));
  memcpy(c->ob_key, key, sizeof(key));
  c->ob_live = true;
  return CVH_OK;
}

// d_u[] takes the level set back (whatever is in flight is settled first).
int one_buffer_leave(cvh_context *c)
{
  if (!c->ob_live) return CVH_OK;
  const int rc = ensure_f64_mirror(c);
  if (rc == CVH_OK) c->ob_live = false;
  return rc;
}

// tiles_y x tiles_x tiles of <= 128 (three channels: 96) rows x 128 columns, at most one per CU.  Pure host arithmetic (also exported for
// the CPU tests: cvh_debug_resident_grid).
bool resident_tile_grid(int h, int w, int channels, int num_cus, int cap_blocks, ResidentGeom *rg)
{
  if ((channels != 1 && channels != 3) || (w & 1) || w < 16 || h < 16) return false;
  const int tw = cvh_resident_tile_w(), thmax = cvh_resident_tile_hmax(channels);
  const int tc = (w + tw - 1) / tw;
  int cap = cap_blocks < CVH_RESIDENT_MAX_TILES ? cap_blocks : CVH_RESIDENT_MAX_TILES;
  if (cap > num_cus) cap = num_cus;                            // one workgroup per CU: a second one on a CU would wait for its slot
  int tr = cap / tc;
  if (tr < 1) return false;
  if (tr > h / 16) tr = h / 16;                                // tiles of >= 16 rows (every wave's band >= 2 rows)
  if ((h + tr - 1) / tr > thmax) return false;                 // does not fit the LDS of the CUs
  rg->tr = tr; rg->tc = tc; rg->band = 0;
  return true;
}

// Does the device launch cooperatively?  Asked once per context; both resident geometries (here, pm_run.hip) size their own kernel by it.
bool launches_cooperatively(cvh_context *c)
{
  if (c->coop_launch < 0) {
    int coop = 0;
    c->coop_launch = hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, c->device) == hipSuccess && coop ? 1 : 0;
  }
  return c->coop_launch != 0;
}

bool resident_geometry(cvh_context *c, ResidentGeom *rg)
{
  // three channels (csv_resident_kernel<3, .>): on request only ("resident" = 1); the automatic choice keeps the per-launch flow
  if (c->C == 3 && c->resident_opt != 1) return false;
  if (!c->resident_opt || (c->C != 1 && c->C != 3) || !use_fast(c) || !c->chain_opt || c->finalize_mode != 0 || (c->w & 1) || c->w < 16 || c->h < 16) return false;
  if (c->state_bits == 32) return false;      // the FP32-state mode is the 2-pixel per-launch kernel's
  if (!(c->kernel == -1 || c->kernel == 2 || c->kernel == 3)) return false;
  // auto: a caller who chose a per-launch data flow or tuned its geometry / launch path gets that flow (measured, one context per size,
  // resident vs per-launch: 128^2 7.4 vs 7.6 us, 256^2 6.9 vs 7.6, 768^2 8.5 vs 9.8, 1024x2048 11.5 vs 14.6, 1536^2 12.4 vs 16.2,
  // 1200x1920 12.0 vs 15.4, 2048^2 16.0 vs 20.9: ahead at every size that fits)
  if (c->resident_opt < 0 && (c->kernel != -1 || c->strip_rows != 0 || c->strips != 0 || !c->use_graph)) return false;
  // auto also steps aside when other contexts stream on this GPU (a batch): cooperative launches of different contexts serialise and cost
  // ~25 us each, while interleaved per-launch flows fill each other's gaps -- measured, eight images interleaved in chunks of 8 iterations
  // (tools/batch_probe.py, gpurun_out/r4s9): 2048^2 32.6 us per image-iteration resident vs 16.2 per launch (17.3 with chunks of 50);
  // 1024^2 22.3 vs 6.1 (10.6).  Decided when a run's first iteration is enqueued, kept for the run.
  // End of round 4, with the resident kernel a quarter faster (12.1 us per iteration at 2048^2): a batch of LARGE planes whose runs are enqueued in
  // LONG chunks is better off with one cooperative launch after the other -- eight planes, us per image-iteration, per-launch interleaved vs
  // resident in chunks of 50 / 100 / 400 (gpurun_out/r4s61, r4s62): 2048^2 16.2 vs 14.7 / 13.2 / 12.1; 1792^2 13.4 vs 13.8 / 12.5 / 11.6;
  // 1536^2 11.0 vs 12.2 / 10.8 / 9.9; 1280^2 8.2 vs 10.5 / 9.2 / 8.3; 1024^2 5.9 vs 8.2 / 6.9 / 6.1.  So in a batch an ENQUEUE takes the resident flow
  // when it is long enough for the plane's size (cvh_run: chunks of up to 1024 iterations) -- per enqueue, not per run: a long warm-up chunk
  // followed by chunks of 8 must not leave a run with 8-iteration cooperative launches (29 us per image-iteration at 2048^2).  The two flows
  // continue each other on one context (sum sets, stop rule, trace); their level sets agree to <= 1e-9, not bit for bit -- a caller who needs
  // the same bits whatever the chunking sets "resident" itself.
  if (c->resident_opt < 0 && !run_is_alone(c)) {
    const double px = (double)c->h * (double)c->w;
    const int need = px >= 3.6e6 ? 48 : px >= 2.9e6 ? 72 : px >= 2.2e6 ? 100 : INT_MAX;
    if (c->run_chunk < need) return false;
  }
  if (c->resident_cap < 0) c->resident_cap = launches_cooperatively(c) ? cvh_resident_blocks_per_cu(c->C) * c->num_cus : 0;
  if (c->resident_cap <= 0) return false;
  return resident_tile_grid(c->h, c->w, c->C, c->num_cus, c->resident_cap, rg);
}

// Class-major workgroup numbering of the wave kernels: workgroups per XCD per dispatch round (0: off), see compute_strip_bounds.
static int class_major_cls(const cvh_context *c, const Geometry &g)
{
  return (((g.strip == 3 && c->wave_cls) || (g.strip == 2 && c->wave_cls == 2)) && c->wave_xcd) ? (c->num_cus >= 8 ? c->num_cus / 8 : 1) : 0;
}

// `step` = index of the launch inside the run (c->enqueued when it is enqueued): selects the chain-mode sum set
void fill_args(const cvh_context *c, CvhStepArgs *a, int in_buf, int step)
{
  memset(a, 0, sizeof(*a));
  a->u_in = c->d_u[in_buf];
  a->u_out = c->d_u[in_buf ^ 1];
  a->state32 = 0;
  if (c->state_bits == 32) {   // FP32 state: the step kernel's pair are the float buffers (prepare() points the initial sums at the mirror)
    a->u_in = reinterpret_cast<const double *>(c->d_uf[in_buf]);
    a->u_out = reinterpret_cast<double *>(c->d_uf[in_buf ^ 1]);
    a->state32 = 1;
  }
  for (int k = 0; k < c->C; ++k) a->img[k] = c->d_img[k];
  a->img_stride = (unsigned)c->img_stride;
  a->st = c->d_state;
  a->partials = c->d_partials;
  a->trace = c->d_trace;
  a->trace_cap = c->trace_cap;
  a->h = c->h; a->w = c->w;
  Geometry g = resolve_geometry(c);
  a->tiles_x = g.tiles_x; a->tiles_y = g.tiles_y;
  a->nparts = g.nblocks;
  a->tile_rows = g.rows;
  a->strip_rows = g.strip_rows;
  a->fused_finalize = c->finalize_mode == 0;
  if (wants_one_buffer(c, g)) {   // the slab is both; in_buf is the parity of the pads and shadow rows the launch reads
    a->u_in = c->d_ob; a->u_out = c->d_ob;
    a->one_buffer = 1;
    a->ob_pitch = cvh_ob_pitch(c->w, g.tiles_x);
    a->ob_rows = cvh_ob_rows(c->h, g.tiles_y);
    a->ob_par = in_buf;
    a->ob_tab = c->d_ob_tab;
  }
  // src/main.cpp:985: dt * (mu*kappa - nu + u_diff/N) evaluates as one addWeighted
  a->alpha = c->p.mu * c->p.dt;
  a->beta = (1.0 / c->C) * c->p.dt;
  a->gamma = -c->p.nu * c->p.dt;
  a->eps = c->p.eps;
  for (int k = 0; k < CVH_MAX_CHANNELS; ++k) { a->lambda1[k] = c->p.lambda1[k]; a->lambda2[k] = c->p.lambda2[k]; }
  const double pi = 3.14159265358979323846;
  a->atan_tab = c->d_atan;
  a->atan2_tab = c->d_atan + 2 * CVH_ATAN_N;
  a->wave_minw = c->wave_minw;
  a->wave_lds_cap = c->wave_lds_cap;
  a->wave_prio = c->wave_prio;
  // workgroup barrier per group of four rows: keeps a workgroup's waves on neighbouring rows (cache locality) -- worth it for one channel;
  // with three channels the barrier costs more than the locality returns (4096^2 x 3, one context: 73.0-74.4 -> 71.9-73.2 us)
  a->wave_sync = c->wave_sync >= 0 ? c->wave_sync : (c->C == 3 ? 0 : 1);
  a->near_switch = c->near_switch;
  a->wave_seam = c->wave_seam;
  a->res_prio = c->res_prio;
  a->res_go_shift = c->res_go_share;
  a->wave_depth = c->wave_depth;
  a->wave_imgv = c->wave_imgv;
  a->dummy = c->d_dummy;
  a->strip_bounds = c->d_bounds;
  a->wave_rev = c->wave_rev;
  a->wave_xcd = c->wave_xcd;
  if (use_chain(c, g)) {
    a->chain = c->d_chain;
    a->chain_pb = c->chain_pb;
    a->chain_phase = (c->chain_pb + step) & 3;
    a->chain_s4 = c->d_partials;   // [2][nparts] rows of sum u_diff^2 (the workspace holds far more)
    // |sum (H - 1/2)| <= N/2 and |sum I (H - 1/2)| <= 255 N / 2 for every subset of pixels: 62 - ceil(log2(bound + 1)) fraction bits
    const double bound[4] = {0.5 * (double)c->n, 127.5 * (double)c->n, 127.5 * (double)c->n, 127.5 * (double)c->n};
    for (int k = 0; k < 4; ++k) {
      int e = 0;
      while (ldexp(1.0, e) < bound[k] + 1.0) ++e;
      a->chain_scale[k] = ldexp(1.0, 62 - e);
      a->chain_inv[k] = ldexp(1.0, e - 62);
    }
  }
  // class-major numbering + class skew: the 2-pixel kernel by default (measured there: -2.3 us at 4096^2); the 1-pixel kernel only
  // on request ("wave_cls" = 2): measured neutral to slightly worse there (4096^2 x 3 channels: 77.2 plain, 77.3 class-major, 82.5 with
  // skew 500; 1 channel: 63.6 / 64.3)
  // write-through stores pay while the ping-pong pair and the planes (mostly) fit the 256 MiB Infinity Cache: up to ~300 MB of footprint
  if (c->wave_pol >= 0) a->wave_pol = c->wave_pol;
  else {   // auto, per run: taken (and re-taken, while nothing of the run is enqueued) from the device's live footprint, then kept
    if (c->run_pol < 0 || c->enqueued == 0) c->run_pol = live_footprint(c) <= 300e6 ? 1 : 0;
    a->wave_pol = c->run_pol;
  }
  a->wave_cls = class_major_cls(c, g);
  a->host_status = c->h_status;
  a->dbg_times = c->d_dbg;
  a->inv_eps = 1.0 / c->p.eps;
  a->dk1 = pi / c->p.eps;
  a->dk2 = pi * c->p.eps;
  far_coef(c->p.eps, c->far_terms, a->far_k, &a->far_thr);
  a->stop_cond = c->stop_cond_h;
  a->npix = (double)c->n;
  for (int k = 0; k < CVH_MAX_CHANNELS; ++k) a->sum_img[k] = c->sum_img[k];
  a->derive_complement = use_fast(c) ? (g.strip >= 2 ? 2 : 1) : 0;  // 2: the wave kernels sum H - 1/2
  a->use_lut = c->use_lut;
  a->use_dma = c->use_dma;
}

// The far-field series of the FAST H_eps (wave_math.h, heaviside_centred_far): k_i = (-1)^i eps^(2i+1) / ((2i+1) pi) and its threshold.
// 5 terms (through t^9/9, t = eps/|u|): next term t^11/11 <= 2.5e-18 for |u| >= 32 eps.  With 4 terms the threshold
// is 64 eps ("far_terms" = 4: k[4] = 0) -- the 4096^2 checkerboard run then spends iterations 3..13 in the near field
// (|u| grows from 36 to 64 there), with 5 terms only iterations 1..2.
void far_coef(double eps, int far_terms, double k[5], double *thr)
{
  const double pi = 3.14159265358979323846;
  const double e = eps, e2 = e * e;
  k[0] = e / pi; k[1] = -(e * e2) / (3.0 * pi);
  k[2] = (e * e2 * e2) / (5.0 * pi); k[3] = -(e * e2 * e2 * e2) / (7.0 * pi);
  k[4] = far_terms == 5 ? (e * e2 * e2 * e2 * e2) / (9.0 * pi) : 0.0;
  *thr = (far_terms == 5 ? 32.0 : 64.0) * e;
}

// Host part of prepare(): the tol-free stop norm of planes that changed on the device.
int prepare_host(cvh_context *c)
{
  if (!c->have_image) return fail(c, CVH_ERR_STATE, "no image set (call cvh_set_image first)");
  if (!c->have_u) return fail(c, CVH_ERR_STATE, "no level set (call cvh_set_levelset or cvh_init_checkerboard first)");
  if (!c->stop_valid) {   // planes changed on the device (Perona-Malik): src/main.cpp:950 uses the smoothed channels
    const int rc = image_stats(c, nullptr);
    if (rc != CVH_OK) return rc;
  }
  c->stop_cond_h = c->p.tol * c->stop_norm;  // :959 (a launch argument: part of the graph key)
  if (c->state_bits == 32 && (!use_fast(c) || resolve_geometry(c).strip != 3))
    return fail(c, CVH_ERR_ARG, "state 32 runs the 2-pixel wave kernel in FAST arithmetic only (math_mode, kernel)");
  return CVH_OK;
}

// Makes c1/c2 of the current level set and the stop condition valid on the device.
int prepare(cvh_context *c)
{
  int rc0 = prepare_host(c);
  if (rc0 != CVH_OK) return rc0;
  // (the stop condition travels as a launch argument, CvhStepArgs::stop_cond: no per-enqueue upload inside the timed interval)
  const bool chain = use_chain(c, resolve_geometry(c));
  if (!c->sums_valid || (chain && !c->chain_acc_valid)) {   // (chain mode: the means exist only as doubles -- another kernel ran --: recompute)
    CvhStepArgs a;
    fill_args(c, &a, current_buffer(c), c->enqueued);
    if (c->state_bits == 32) {   // the sums of the level set the run starts from are taken of its double mirror (the rounded values)
      const int rc = ensure_f64_mirror(c);
      if (rc != CVH_OK) return rc;
      a.u_in = c->d_u[current_buffer(c)];
    }
    if (a.one_buffer) {   // one-buffer flow: of the dense mirror as well
      const int rc = ensure_f64_mirror(c);
      if (rc != CVH_OK) return rc;
      a.u_in = c->d_u[current_buffer(c)];
    }
    int nparts = 0;
    HIPCHK(c, cvh_launch_init_sums(a, c->C, use_fast(c), &nparts, c->stream));
    a.nparts = nparts;
    HIPCHK(c, cvh_launch_finalize(a, c->C, 1, c->stream));   // chain mode: also seeds the fixed-point set of this step
    sums_taken(c, chain);
  }
  return CVH_OK;
}

// Wave kernel: rows [bounds[k], bounds[k+1]) belong to strip k.  All waves start together, but at
// equal priority the SIMD arbiter favours the OLDEST wave, i.e. the lowest workgroup index, and
// equal strips then finish up to 10 us apart inside one SIMD (tools/wave_timeline.py) -- the tail
// runs at 1-2 waves per SIMD.  wave_skew = 1000 alpha makes the strip length fall linearly from
// (1 + alpha) to (1 - alpha) times the mean with the strip index, so they finish together.
// First row of every strip of the wave kernels, b[0 .. S] (pure host arithmetic: also exported for the CPU tests).
//   kind 3: 2-pixel kernel (a workgroup is 2 wave-columns of 2 strips), kind 2: 1-pixel kernel (4 wave-columns of ONE strip)
//   cls > 0: class-major workgroup numbering with `cls` workgroups per XCD per dispatch round; cskew = per-mille skew between rounds
//   cls == 0: equal strips of strip_rows rows (skew: the 1-pixel kernel's legacy linear skew)
void compute_strip_bounds(int kind, int h, int tiles_x, int S, int strip_rows, int nblocks, int cls, int cskew, int skew,
                          std::vector<int> &b)
{
  b.assign((size_t)S + 1, 0);
  if (cls) {
    // Class-major numbering (csv_wave2_kernel.hip): the hardware deals workgroup b to XCD b % 8 and, inside an XCD, the first
    // `cls` workgroups to distinct CUs, the next `cls` to the same CUs again, ... (measured, tools/wave_timeline.py: a CU holds
    // workgroups j, j + 32, j + 64 of its XCD, in wave slots 0, 1, 2).  At equal priority the SIMD arbiter serves the OLDEST
    // wave first, so round 0 finishes 4 us before round 1 and 8 us before round 2 (53 / 57 / 61 us) and the tail of every launch
    // runs at 2, then 1 wave per SIMD.  The class-major numbering makes the strips of one round contiguous, and cskew = 1000 a
    // gives the rounds (1 + a), 1, (1 - a) times the mean strip length.  Rows are dealt by cumulative weight: no short last strip.
    const int spw = kind == 3 ? 2 : 1;
    const int nbc = kind == 3 ? (tiles_x + 1) / 2 : (tiles_x + 3) / 4, nb = nblocks, q = nb >> 3, r = nb & 7;
    const int npairs = (S + spw - 1) / spw;
    int ncls = 0;
    std::vector<long> K;                       // K[k] = workgroups in rounds 0..k
    for (;; ++ncls) {
      long tot = 0;
      for (int x = 0; x < 8; ++x) { const int nx = q + (x < r ? 1 : 0); const long lim = (long)(ncls + 1) * cls; tot += nx < lim ? nx : lim; }
      K.push_back(tot);
      if (tot >= nb) { ++ncls; break; }
    }
    const double a_ = cskew / 1000.0, mid = (ncls - 1) / 2.0;
    std::vector<double> wgt((size_t)S);
    double total = 0;
    for (int sp = 0; sp < npairs; ++sp) {
      const long rank = (long)sp * nbc + nbc / 2;
      int k = 0;
      while (k < ncls - 1 && rank >= K[k]) ++k;
      const double wv = 1.0 + a_ * (mid - k) / (mid > 0 ? mid : 1.0);
      for (int t = 0; t < spw && spw * sp + t < S; ++t) { wgt[spw * sp + t] = wv; total += wv; }
    }
    double cum = 0;
    for (int k = 0; k < S; ++k) { b[k] = (int)((double)h * (cum / total) + 0.5); cum += wgt[k]; }
    for (int k = 1; k < S; ++k) if (b[k] < b[k - 1]) b[k] = b[k - 1];
  } else {
    const double alpha = skew / 1000.0;
    for (int k = 0; k <= S; ++k) {
      long v;
      if (skew == 0) v = (long)k * strip_rows;
      else { const double x = (double)k / S; v = (long)((double)h * (x + alpha * x * (1.0 - x))); }
      b[k] = (int)(v < h ? v : h);
    }
  }
  b[S] = h;
}

int upload_strip_bounds(cvh_context *c, const Geometry &g)
{
  const int cls = class_major_cls(c, g);
  const bool alone = run_is_alone(c);
  const int key[4] = {g.tiles_y, g.strip_rows, c->wave_skew + 1000 * (cls ? c->wave_cskew + 1 : 0) + 10000000 * g.strip + (c->state_bits == 32 ? 500000000 : 0) + (alone ? 0 : 250000000), c->h};
  if (!memcmp(key, c->bounds_key, sizeof(key))) return CVH_OK;
  std::vector<int> b;
  // The skew pays for short strips only (one process, 2-pixel kernel: 4096^2, 46 rows: 61.1 -> 58.7 us; 6144^2, 102 rows: 140.9 ->
  // 140.6; 8192^2 forced onto this kernel, 178 rows: 244 -> 285 us): full below 46 rows, fading to none at 128.
  int cskew = c->wave_cskew;
  if (g.strip_rows > 46) cskew = g.strip_rows >= 128 ? 0 : (int)(cskew * (128.0 - g.strip_rows) / (128.0 - 46.0));
  // three channels: round 3 measured equal strips best (73.3 vs 74.1 us with the full skew, with the workgroup barrier per group); without that
  // barrier (their default since) the wave timeline shows the staircase again -- strips of dispatch round 0 end at 65 us, of round 2 at 74-76 -- and
  // a skew of 0.425 wins: five alternations in one context (round 4, gpurun_out/r4s17) 73.00 (equal) / 71.69 (0.35) / 70.88 (0.425) / 71.74 (0.5 +
  // priority scheme 2) us.  Any other "wave_cskew" applies as given.
  // (the FP32-state flavour of three channels, compute-bound, still prefers equal strips: 52.5 vs 54.6 us, gpurun_out/r4s19)
  if (c->C == 3 && c->wave_cskew == 500) cskew = c->state_bits == 32 ? 0 : 425;
  // a batch: launches of several contexts interleave on the CUs, the staircase of ONE launch's dispatch rounds is not what ends a launch any more --
  // equal strips (8 interleaved 4096^2 images, `bench.py --config C5`: 298.1 k against 293.2-293.4 k Mpixel-iterations/s, gpurun_out/r4s23)
  if (!alone && c->wave_cskew == 500) cskew = 0;
  compute_strip_bounds(g.strip, c->h, g.tiles_x, g.tiles_y, g.strip_rows, g.nblocks, cls, cskew, c->wave_skew, b);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // launches already enqueued read the old table
  HIPCHK(c, hipMemcpy(c->d_bounds, b.data(), b.size() * sizeof(int), hipMemcpyHostToDevice));
  c->h_bounds = b;
  memcpy(c->bounds_key, key, sizeof(key));
  return CVH_OK;
}

// `capturing`: the launch is recorded into a stream capture, nothing reaches the GPU -- the context's bookkeeping of what is
// in flight (steps_enqueued) is updated by the caller when the graph is really launched
int launch_one_step(cvh_context *c, int in_buf, int step, bool capturing, CvhLaunchNote *note)
{
  CvhStepArgs a;
  fill_args(c, &a, in_buf, step);
  a.note = note;
  const int kind = resolve_geometry(c).strip;
  if (kind == 3) HIPCHK(c, cvh_launch_wave2(a, c->C, use_fast(c), c->stream));
  else if (kind == 2) HIPCHK(c, cvh_launch_wave(a, c->C, use_fast(c), c->stream));
  else HIPCHK(c, cvh_launch_step(a, c->C, use_fast(c), c->stream));
  if (note) return CVH_OK;
  if (c->finalize_mode == 1) HIPCHK(c, cvh_launch_finalize(a, c->C, 0, c->stream));
  if (!capturing) steps_enqueued(c, 1, a.nparts, a.chain != nullptr, false);
  return CVH_OK;
}

// Chain mode: the last launch's iteration has no successor to book it -- one small kernel does (norm, stop rule,
// trace row) and writes the region means of the current level set into the state block.
static int chain_flush(cvh_context *c)
{
  if (!c->chain_pending) return CVH_OK;
  CvhStepArgs a;
  fill_args(c, &a, 0, 0);
  if (!a.chain) return fail(c, CVH_ERR_STATE, "chain-mode launches are pending but the context no longer selects chain mode");
  if (c->pending_nparts > 0) a.nparts = c->pending_nparts;   // the rows the pending launch left (a fused batch's grid may differ)
  HIPCHK(c, cvh_launch_chain_flush(a, c->C, c->stream));
  c->chain_pending = false;
  return CVH_OK;
}

// The pending iteration of a per-launch wave kernel is booked by the next launch's bookkeeper only if that launch runs on the same
// grid (its rows of sum u_diff^2 are read by workgroup count); before anything else -- a resident launch (nparts < 0), which never
// books it (it used to lose that iteration's norm, trace row and stop test), or a grid of another size (a fused batch's share of the
// chip, a context's own grid after one) -- the flush kernel books it, exactly as a cvh_sync in between would.
int flush_for_grid(cvh_context *c, int nparts)
{
  if (c->chain_pending && c->pending_nparts > 0 && c->pending_nparts != nparts) return chain_flush(c);
  return CVH_OK;
}

// A run of kGraphSteps consecutive steps as one hipGraph (launch arguments differ between steps only
// in the ping-pong parity; step counter, trace row and stop flag live on the device).  Measured on
// MI355X: back-to-back launches on a stream cost 2.8 us each, graph nodes 1.6 us (tools/launch_probe.hip).
// The instantiated graph is kept per start parity and rebuilt when any launch argument changed.
static int ensure_step_graph(cvh_context *c, int parity)
{
  // One slot per sum-set phase of the first step: a chunk size that is not a multiple of 4 (sync_every = 18, repeated
  // cvh_enqueue_steps(18), a run that stopped early) cycles through the phases, and each keeps its instantiated graph.
  StepGraph &g = c->graphs[(c->chain_pb + c->enqueued) & 3];
  // the arguments of consecutive steps differ in the ping-pong parity and the chain-mode sum set: period 4
  CvhStepArgs key[4];
  for (int s = 0; s < 4; ++s) fill_args(c, &key[s], parity ^ (s & 1), c->enqueued + s);
  const int kind = resolve_geometry(c).strip, flavour = (use_fast(c) ? 1 : 0) | (c->finalize_mode << 1);
  if (g.exec && g.kind == kind && g.flavour == flavour && !memcmp(key, g.key, sizeof(key))) return CVH_OK;
  if (g.exec) {   // an argument changed: the old exec may still have launches in flight (cvh_run queues chunks ahead)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipGraphExecDestroy(g.exec);
    g.exec = nullptr;
  }
  const int rc = capture_graph(c, &g.exec, [&] {
    int r = CVH_OK;
    for (int s = 0; s < kGraphSteps && r == CVH_OK; ++s) r = launch_one_step(c, parity ^ (s & 1), c->enqueued + s, true);
    return r;
  }, "hipStreamEndCapture: %s");
  if (rc != CVH_OK) return rc;
  memcpy(g.key, key, sizeof(key));
  g.kind = kind; g.flavour = flavour;
  return CVH_OK;
}

// One-off HOST work of a run: the strip table and, when the run is long enough to use them, the
// instantiated graph of the run's ping-pong parity (stream capture + hipGraphInstantiate cost about a
// millisecond each while the GPU idles).  Called before the timed interval opens, so that neither
// cvh_last_run_ms nor a caller's wall clock around cvh_enqueue_steps / cvh_sync is charged with it.
static int warm_impl(cvh_context *c, long nsteps)
{
  if (nsteps > 0) c->run_chunk = (int)(nsteps < 1024 ? nsteps : 1024);   // (the caller announces its next enqueue)
  { ResidentGeom rg; if (resident_geometry(c, &rg)) return one_buffer_leave(c); }   // one cooperative launch per chunk: nothing to capture
  const Geometry g = resolve_geometry(c);
  if (g.strip >= 2) { const int rc = upload_strip_bounds(c, g); if (rc != CVH_OK) return rc; }
  { const int rc = one_buffer_flow(c, g); if (rc != CVH_OK) return rc; }
  if (c->use_graph && nsteps >= kGraphSteps) {
    // every graph launch of one call starts on the same ping-pong parity / sum-set phase (kGraphSteps is a multiple of 4),
    // after the nsteps % kGraphSteps plain launches that enqueue_impl() issues first
    const int ahead = (int)(nsteps % kGraphSteps);
    c->enqueued += ahead;
    const int rc = ensure_step_graph(c, (c->cur_base + c->enqueued) & 1);
    c->enqueued -= ahead;
    if (rc != CVH_OK) return rc;
  }
  return CVH_OK;
}

// Synchronisation words and border buffer of the resident kernels (csv_resident_kernel.hip, pm_resident_kernel.hip), pinned error word.
int ensure_resident_buffers(cvh_context *c)
{
  if (c->d_resident) return CVH_OK;
  const int halo = cvh_resident_halo_doubles();
  // (fine-grained and uncached device memory -- hipExtMallocWithFlags -- for these lines and buffers were tried: no difference,
  // profiles/r04_C4/resident_memory_kinds.txt)
  HIPCHK(c, hipMalloc((void **)&c->d_resident, sizeof(CvhResident)));
  HIPCHK(c, hipMalloc((void **)&c->d_res_halo, (size_t)2 * CVH_RESIDENT_MAX_TILES * halo * sizeof(double)));
  HIPCHK(c, hipHostMalloc((void **)&c->h_resident, 64, hipHostMallocDefault));
  memset(c->h_resident, 0, 64);
  return CVH_OK;
}

// One cooperative launch per chunk of iterations (csv_resident_kernel.hip).
int launch_resident(cvh_context *c, const ResidentGeom &rg, int nsteps, CvhLaunchNote *note)
{
  const int ntiles = rg.tr * rg.tc;
  if (!note) { const int rc = ensure_resident_buffers(c); if (rc != CVH_OK) return rc; }
  if (!note) { const int rc = one_buffer_leave(c); if (rc != CVH_OK) return rc; }
  if (!note) { const int rc = flush_for_grid(c, -1); if (rc != CVH_OK) return rc; }
  constexpr int kMaxPerLaunch = 4096;
  for (int s = 0; s < nsteps || note;) {
    const int n = nsteps - s < kMaxPerLaunch ? nsteps - s : kMaxPerLaunch;
    CvhStepArgs a;
    fill_args(c, &a, (c->cur_base + c->enqueued) & 1, c->enqueued);
    if (!a.chain) return fail(c, CVH_ERR_STATE, "resident mode needs chain-mode sums");
    a.tiles_x = rg.tc; a.tiles_y = rg.tr; a.nparts = ntiles;
    {   // every tile 16, 32, 64 or 128 rows (three channels: up to 64): the straight-line flavour of the march
      const int th = c->h % rg.tr == 0 ? c->h / rg.tr : 0;
      a.res_band_rows = (c->res_straight && (th == 16 || th == 32 || th == 64 || th == 128) && th <= cvh_resident_tile_hmax(c->C)) ? th / 8 : 0;
    }
    a.resident = c->d_resident;
    a.res_halo = c->d_res_halo;
    a.res_steps = n;
    a.res_t0 = c->enqueued;
    a.res_poll_cap = 2000000;      // seconds of polling before a wait gives up (the grid always drains)
    a.note = note;
    if (note) { HIPCHK(c, cvh_launch_resident(a, c->C, c->stream)); return CVH_OK; }
    HIPCHK(c, hipMemsetAsync(c->d_resident, 0, c->C == 1 ? CVH_RESIDENT_C1_BYTES : sizeof(CvhResident), c->stream));
    HIPCHK(c, cvh_launch_resident(a, c->C, c->stream));
    steps_enqueued(c, n, ntiles, true, true);
    s += n;
  }
  return CVH_OK;
}

static int enqueue_impl(cvh_context *c, int nsteps)
{
  if (nsteps > 0) c->run_chunk = nsteps;        // (resident_geometry's rule for a batch looks at the length of THIS enqueue)
  {
    ResidentGeom rg;
    if (resident_geometry(c, &rg)) return launch_resident(c, rg, nsteps, nullptr);
    const Geometry g = resolve_geometry(c);
    if (g.strip >= 2) { const int rc = upload_strip_bounds(c, g); if (rc != CVH_OK) return rc; }
    { const int rc = one_buffer_flow(c, g); if (rc != CVH_OK) return rc; }
    const int rc = flush_for_grid(c, g.nblocks);
    if (rc != CVH_OK) return rc;
  }
  // The odd-sized part goes FIRST as plain launches: from an idle stream they reach the GPU within 3-5 us, while the first
  // hipGraph replay takes 10-16 us; the graphs (runs of kGraphSteps) follow.  warm_impl() builds the graph for that position.
  int s = 0;
  const int plain = (c->use_graph && nsteps >= kGraphSteps) ? nsteps % kGraphSteps : nsteps;
  for (; s < plain; ++s) {
    const int rc = launch_one_step(c, (c->cur_base + c->enqueued) & 1, c->enqueued);
    if (rc != CVH_OK) return rc;
  }
  while (nsteps - s >= kGraphSteps) {
    const int parity = (c->cur_base + c->enqueued) & 1;
    const int rc = ensure_step_graph(c, parity);
    if (rc != CVH_OK) return rc;
    const StepGraph &sg = c->graphs[(c->chain_pb + c->enqueued) & 3];
    HIPCHK(c, hipGraphLaunch(sg.exec, c->stream));
    steps_enqueued(c, kGraphSteps, sg.key[0].nparts, sg.key[0].chain != nullptr, false);
    s += kGraphSteps;
  }
  return CVH_OK;
}

extern "C" int cvh_enqueue_steps(cvh_context *c, int nsteps)
{
  if (!c || nsteps < 0) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = prepare_host(c);
  if (rc != CVH_OK) return rc;
  rc = warm_impl(c, nsteps);   // graph build etc. stays outside the timed interval
  if (rc != CVH_OK) return rc;
  if (!c->timing_open) {
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    c->timing_open = true;
  }
  rc = prepare(c);
  if (rc != CVH_OK) return rc;
  return enqueue_impl(c, nsteps);
}

extern "C" int cvh_warm(cvh_context *c, int nsteps)
{
  if (!c || nsteps < 0) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = prepare_host(c);
  if (rc != CVH_OK) return rc;
  return warm_impl(c, nsteps);
}

int sync_impl(cvh_context *c)
{
  const bool via_flush = c->chain_pending;   // the flush kernel writes {steps_done, stopped, norm} into the pinned host block itself
  int rc = chain_flush(c);
  if (rc != CVH_OK) return rc;
  if (c->timing_open) HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  if (!via_flush) HIPCHK(c, hipMemcpyAsync(&c->h_state[0], c->d_state, sizeof(CvhState), hipMemcpyDeviceToHost, c->stream));
  if (c->resident_used) HIPCHK(c, hipMemcpyAsync(c->h_resident, c->d_resident, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->resident_used) {
    c->resident_used = false;
    if (c->h_resident[0]) {
      c->timing_open = false;
      return fail(c, CVH_ERR_HIP, "the resident step kernel gave up waiting for a workgroup: the level set of this run is invalid");
    }
  }
  if (via_flush) {
    c->h_state[0].steps_done = c->h_status[0];
    c->h_state[0].stopped = c->h_status[1];
    memcpy(&c->h_state[0].norm, &c->h_status[2], sizeof(double));
  }
  if (c->timing_open) {
    HIPCHK(c, hipEventElapsedTime(&c->last_run_ms, c->ev0, c->ev1));
    c->timing_open = false;
  }
  c->steps_done = c->h_state[0].steps_done;
  c->enqueued = c->steps_done;   // everything enqueued has run, and launches past a stop were no-ops
  return CVH_OK;
}

extern "C" int cvh_sync(cvh_context *c, int *steps_done_total, double *last_norm, int *stopped)
{
  if (!c) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = sync_impl(c);
  if (rc != CVH_OK) return rc;
  if (steps_done_total) *steps_done_total = c->h_state[0].steps_done;
  if (last_norm) *last_norm = c->h_state[0].norm;
  if (stopped) *stopped = c->h_state[0].stopped;
  return CVH_OK;
}

extern "C" int cvh_run(cvh_context *c, int max_steps, int *steps_done, double *last_norm)
{
  if (!c) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->have_image) return fail(c, CVH_ERR_STATE, "no image set (call cvh_set_image first)");
  if (!c->have_u) return fail(c, CVH_ERR_STATE, "no level set (call cvh_set_levelset or cvh_init_checkerboard first)");
  int rc = reset_run_impl(c);   // settles whatever is in flight first
  if (rc != CVH_OK) return rc;
  long remaining = max_steps < 0 ? (long)INT_MAX : (long)max_steps;  // src/main.cpp:890
  rc = prepare_host(c);  // one-off host work (src/main.cpp:950-959) stays outside the device timing
  if (rc != CVH_OK) return rc;
  rc = warm_impl(c, remaining < c->sync_every ? remaining : (long)c->sync_every);  // so do the strip table and the graph of the first chunk
  if (rc != CVH_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  rc = prepare(c);
  if (rc != CVH_OK) return rc;
  // Chunks of sync_every launches.  The finalising workgroup of every step stores
  // {steps_done, stopped} into pinned host memory; the host reads those two words between
  // chunks (no copy, no synchronisation) and never runs more than kAhead chunks in front of
  // the device.  Launches queued behind a fired stop are no-ops on the device (sticky flag).
  constexpr int kAhead = 4;
  volatile int *hs = c->h_status;
  bool stopped = false;
  int queued = 0;
  // resident mode: a chunk is ONE launch that loads the tiles, iterates and stores them; the stop rule ends it inside the kernel at the
  // reference's iteration, so chunks can be long (the tile load / store of a 2048^2 plane is worth ~0.4 us per iteration at 32)
  int chunk_len = c->sync_every;
  c->run_chunk = (int)(remaining < 1024 ? remaining : 1024);     // (what a chunk is if the run takes the resident flow: resident_geometry's rule for a batch)
  { ResidentGeom rg; if (resident_geometry(c, &rg) && chunk_len < 1024) chunk_len = 1024; else c->run_chunk = chunk_len; }
  while (remaining > 0 && !stopped) {
    while (queued - hs[0] > kAhead * chunk_len && !hs[1]) {
      if (hipStreamQuery(c->stream) == hipSuccess) break;  // everything queued has run
    }
    if (hs[1]) { stopped = true; break; }
    const int chunk = (int)(remaining < chunk_len ? remaining : chunk_len);
    rc = enqueue_impl(c, chunk);
    if (rc != CVH_OK) return rc;
    remaining -= chunk;
    queued += chunk;
  }
  c->timing_open = true;   // sync_impl closes the interval opened at ev0 (after the chain-mode flush)
  rc = sync_impl(c);
  if (rc != CVH_OK) return rc;
  if (steps_done) *steps_done = c->h_state[0].steps_done;
  if (last_norm) *last_norm = c->h_state[0].norm;
  return CVH_OK;
}

