// api.hip — host side of the C ABI declared in include/chanvese_hip.h: context lifecycle, options, image and level-set I/O, getters.
// and the transitions of a context's run state.  The flows live in csv_run.hip (CSV steps of one context), csv_batch.hip (fused batch),
// pm_run.hip (Perona-Malik), io_run.hip (device memory, and the member-table calls every small device operation goes through:
// cvh_init_checkerboard is there, cvh_get_mask here is mask_out into the context's buffer), init_run.hip (device-side initial level
// sets); never throws.
#include "cvh_host.h"

// cvh_last_error(NULL): per host thread, the calling thread's own last context-less error.  Reached through create_err() alone, so that
// no other unit addresses the thread-local storage itself.
static thread_local char g_create_err[kErrLen] = "no error";
char *create_err() { return g_create_err; }

int fail(cvh_context *ctx, int code, const char *fmt, ...)
{
  char *dst = ctx ? ctx->err : g_create_err;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(dst, 512, fmt, ap);
  va_end(ap);
  return code;
}

extern "C" const char *cvh_version(void) { return "chanvese_hip 0.1 (gfx950)"; }

void cvh_fill_note(CvhLaunchNote *note, unsigned grid, unsigned block, size_t lds, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(note->name, sizeof(note->name), fmt, ap);
  va_end(ap);
  note->grid = grid; note->block = block; note->lds = (unsigned)lds;
}

// The atan tables of the FAST flavour, rounded once from long double: atan(i/128) and pi/2 - atan(i/128) (atan_table), then
// (pi/4 + atan((j-128)/128)) / pi (heaviside_centred_near).  tab holds 2 * CVH_ATAN_N + CVH_ATAN2_N doubles.
void fill_atan_tables(double *tab)
{
  const long double pil = 3.14159265358979323846264338327950288L;
  for (int i = 0; i < CVH_ATAN_N; ++i) {
    const long double at = atanl((long double)i / (CVH_ATAN_N - 1));
    tab[i] = (double)at;
    tab[CVH_ATAN_N + i] = (double)(pil / 2 - at);
  }
  for (int j = 0; j < CVH_ATAN2_N; ++j)
    tab[2 * CVH_ATAN_N + j] = (double)((pil / 4 + atanl((long double)(j - 128) / 128)) / pil);
}

extern "C" void cvh_default_params(cvh_params *p)
{
  if (!p) return;
  p->mu = 0.5; p->nu = 0.0; p->dt = 1.0; p->eps = 1.0; p->tol = 0.001;  // src/main.cpp:759-765
  for (int k = 0; k < CVH_MAX_CHANNELS; ++k) { p->lambda1[k] = 1.0; p->lambda2[k] = 1.0; }
}

extern "C" int cvh_device_count(int *count)
{
  if (!count) return CVH_ERR_ARG;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return fail(nullptr, CVH_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
  *count = n;
  return CVH_OK;
}

extern "C" const char *cvh_last_error(const cvh_context *ctx) { return ctx ? ctx->err : g_create_err; }

static int check_params(cvh_context *ctx, const cvh_params *p, int C)
{
  // the reference's range checks, src/main.cpp:795-830
  if (!(p->dt > 0)) return fail(ctx, CVH_ERR_ARG, "Cannot have negative or zero timestep: %f.", p->dt);
  if (p->mu < 0) return fail(ctx, CVH_ERR_ARG, "Length penalty parameter cannot be negative: %f.", p->mu);
  for (int k = 0; k < C; ++k) {
    if (p->lambda1[k] < 0) return fail(ctx, CVH_ERR_ARG, "The value of lambda1 cannot be negative.");
    if (p->lambda2[k] < 0) return fail(ctx, CVH_ERR_ARG, "The value of lambda2 cannot be negative.");
  }
  return CVH_OK;
}

// Every live context of the process (cvh_create .. cvh_destroy).  Several contexts on one GPU share its 256 MiB Infinity Cache: what one
// context's footprint suggests (write-through stores while its ping-pong pair fits the cache) is wrong when eight of them stream side by
// side -- the batch BASELINE configs[4] describes.  Round 3 left that to the caller ("wave_pol" = 0); now the automatic choice looks here.
static std::mutex g_live_mu;
static std::vector<cvh_context *> g_live;

// bytes per pixel-iteration pair (level-set ping-pong + planes) of every context on c's device that holds an image and a level set and
// streams beside the others ("co_resident")
static int live_contexts(const cvh_context *c)
{
  std::lock_guard<std::mutex> lk(g_live_mu);
  int k = 0;
  for (const cvh_context *o : g_live)
    if (o->device == c->device && o->co_resident && ((o->have_u && o->have_image) || o == c)) ++k;
  return k;
}

// Is this context the only co-resident one on its device?  Decided when a run's first iteration is enqueued, kept for the run.
bool run_is_alone(const cvh_context *c)
{
  if (c->run_alone < 0 || c->enqueued == 0) c->run_alone = live_contexts(c) <= 1 ? 1 : 0;
  return c->run_alone != 0;
}

double live_footprint(const cvh_context *c)
{
  std::lock_guard<std::mutex> lk(g_live_mu);
  double sum = 0.0;
  for (const cvh_context *o : g_live)
    if (o->device == c->device && o->co_resident && ((o->have_u && o->have_image) || o == c))
      sum += (double)o->n * (2.0 * (o->state_bits / 8) + o->C);
  return sum;
}

extern "C" void cvh_destroy(cvh_context *c)
{
  if (!c) return;
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live.erase(std::remove(g_live.begin(), g_live.end(), c), g_live.end());
  }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->d_img_slab) (void)hipFree(c->d_img_slab);
  if (c->d_u_slab) (void)hipFree(c->d_u_slab);
  if (c->d_ob) (void)hipFree(c->d_ob);
  if (c->d_ob_tab) (void)hipFree(c->d_ob_tab);
  if (c->d_uf_slab) (void)hipFree(c->d_uf_slab);
  for (int k = 0; k < 2; ++k) if (c->d_pm[k]) (void)hipFree(c->d_pm[k]);
  if (c->d_state) (void)hipFree(c->d_state);
  if (c->h_state) (void)hipHostFree(c->h_state);
  if (c->d_partials) (void)hipFree(c->d_partials);
  if (c->d_trace) (void)hipFree(c->d_trace);
  if (c->d_mask) (void)hipFree(c->d_mask);
  if (c->d_atan) (void)hipFree(c->d_atan);
  if (c->d_dbg) (void)hipFree(c->d_dbg);
  for (int k = 0; k < 4; ++k) if (c->graphs[k].exec) (void)hipGraphExecDestroy(c->graphs[k].exec);
  if (c->pm_graph) (void)hipGraphExecDestroy(c->pm_graph);
  if (c->d_dummy) (void)hipFree(c->d_dummy);
  if (c->d_chain) (void)hipFree(c->d_chain);
  if (c->d_resident) (void)hipFree(c->d_resident);
  if (c->d_res_halo) (void)hipFree(c->d_res_halo);
  if (c->d_pm_halo) (void)hipFree(c->d_pm_halo);
  free_table(&c->pm_batch);
  free_table(&c->io_table);
  if (c->h_io) (void)hipHostFree(c->h_io);
  if (c->d_reinit) (void)hipFree(c->d_reinit);
  if (c->d_cc) (void)hipFree(c->d_cc);
  for (DeviceTable *t : {&c->cc_table, &c->regions, &c->contour_edges, &c->contour_points, &c->overlap}) free_table(t);
  if (c->d_contour) (void)hipFree(c->d_contour);
  if (c->d_hist) (void)hipFree(c->d_hist);
  if (c->d_energy) (void)hipFree(c->d_energy);
  if (c->d_score) (void)hipFree(c->d_score);
  if (c->d_morph) (void)hipFree(c->d_morph);
  if (c->d_split) (void)hipFree(c->d_split);
  if (c->d_local) (void)hipFree(c->d_local);
  if (c->d_rank) (void)hipFree(c->d_rank);
  if (c->d_smooth) (void)hipFree(c->d_smooth);
  if (c->d_overlap_plane) (void)hipFree(c->d_overlap_plane);
  if (c->d_multiphase) (void)hipFree(c->d_multiphase);
  free_table(&c->mp_trace);
  if (c->d_localized) (void)hipFree(c->d_localized);
  free_table(&c->loc_trace);
  if (c->d_gq) (void)hipFree(c->d_gq);
  if (c->d_geodesic) (void)hipFree(c->d_geodesic);
  free_table(&c->geo_trace);
  if (c->d_convex) (void)hipFree(c->d_convex);
  free_table(&c->cvx_trace);
  free_table(&c->march_table);
  if (c->h_march) (void)hipHostFree(c->h_march);
  if (c->ev_io_in) (void)hipEventDestroy(c->ev_io_in);
  if (c->ev_io_out) (void)hipEventDestroy(c->ev_io_out);
  if (c->h_resident) (void)hipHostFree(c->h_resident);
  if (c->d_bounds) (void)hipFree(c->d_bounds);
  if (c->h_status) (void)hipHostFree(c->h_status);
  if (c->d_isums) (void)hipFree(c->d_isums);
  if (c->h_isums) (void)hipHostFree(c->h_isums);
  batch_cache_free(c);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  for (int k = 0; k < 4; ++k) if (c->evp[k]) (void)hipEventDestroy(c->evp[k]);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

static int create_impl(cvh_context *c)
{
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && cus > 0) c->num_cus = cus;
  }
  // one slab for the planes: the 1-pixel wave kernel fetches a group's image pieces of all channels with one instruction
  c->img_stride = (c->n + 255) & ~(size_t)255;
  HIPCHK(c, hipMalloc((void **)&c->d_img_slab, c->img_stride * c->C));
  for (int k = 0; k < c->C; ++k) c->d_img[k] = c->d_img_slab + (size_t)k * c->img_stride;
  {
    // one slab for the ping-pong pair (64 doubles of slack behind each buffer: the wave kernels park the stores of lanes
    // that own no pixel there).  Skewing the second buffer against the first by 256 B .. 1 MiB was measured: no effect.
    const size_t each = (((c->n + 64) * sizeof(double)) + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    HIPCHK(c, hipMalloc((void **)&c->d_u_slab, 2 * each));
    c->d_u[0] = (double *)c->d_u_slab;
    c->d_u[1] = (double *)((char *)c->d_u_slab + each);
  }
  HIPCHK(c, hipMalloc((void **)&c->d_state, sizeof(CvhState)));
  HIPCHK(c, hipMemset(c->d_state, 0, sizeof(CvhState)));
  HIPCHK(c, hipHostMalloc((void **)&c->h_state, 4 * sizeof(CvhState), hipHostMallocDefault));
  memset(c->h_state, 0, 4 * sizeof(CvhState));
  int step_blocks = cvh_step_max_blocks(c->h, c->w);
  {
    const int wave_blocks = (((c->w + cvh_wave_cols() - 1) / cvh_wave_cols() + 3) / 4) * c->h + 1;  // strip_rows >= 1
    if (wave_blocks > step_blocks) step_blocks = wave_blocks;
  }
  {
    double tab[2 * CVH_ATAN_N + CVH_ATAN2_N];
    fill_atan_tables(tab);
    HIPCHK(c, hipMalloc((void **)&c->d_atan, sizeof(tab)));
    HIPCHK(c, hipMemcpy(c->d_atan, tab, sizeof(tab), hipMemcpyHostToDevice));
  }
  const int init_blocks = cvh_init_sum_blocks(c->h, c->w);
  c->partial_rows = step_blocks > init_blocks ? step_blocks : init_blocks;
  HIPCHK(c, hipMalloc((void **)&c->d_partials, (size_t)c->partial_rows * cvh_nsums(c->C) * sizeof(double)));
  HIPCHK(c, hipMalloc((void **)&c->d_dummy, (size_t)(c->w > 64 ? c->w : 64) * sizeof(double)));
  HIPCHK(c, hipMalloc((void **)&c->d_bounds, (size_t)(c->h + 2) * sizeof(int)));
  HIPCHK(c, hipMalloc((void **)&c->d_chain, sizeof(CvhChainAcc)));
  HIPCHK(c, hipMemset(c->d_chain, 0, sizeof(CvhChainAcc)));
  HIPCHK(c, hipHostMalloc((void **)&c->h_status, 64, hipHostMallocMapped));
  c->h_status[0] = 0; c->h_status[1] = 0;
  HIPCHK(c, hipMalloc((void **)&c->d_isums, 8 * sizeof(unsigned long long)));
  HIPCHK(c, hipHostMalloc((void **)&c->h_isums, 8 * sizeof(unsigned long long), hipHostMallocDefault));
  HIPCHK(c, hipEventCreate(&c->ev0));
  HIPCHK(c, hipEventCreate(&c->ev1));
  for (hipEvent_t *ev : {&c->evp[0], &c->evp[1], &c->evp[2], &c->evp[3], &c->ev_join, &c->ev_io_in, &c->ev_io_out})
    HIPCHK(c, hipEventCreateWithFlags(ev, hipEventDisableTiming));
  snprintf(c->err, sizeof(c->err), "no error");
  return CVH_OK;
}

extern "C" int cvh_create(cvh_context **out, int h, int w, int channels, const cvh_params *p, int device)
{
  if (!out) return fail(nullptr, CVH_ERR_ARG, "cvh_create: out is NULL");
  *out = nullptr;
  if (h <= 0 || w <= 0) return fail(nullptr, CVH_ERR_ARG, "cvh_create: image size must be positive (got %d x %d)", h, w);
  if (channels != 1 && channels != 3)
    return fail(nullptr, CVH_ERR_ARG, "cvh_create: channels must be 1 (grayscale) or 3 (colour), got %d", channels);
  cvh_params def;
  cvh_default_params(&def);
  if (!p) p = &def;
  int rc = check_params(nullptr, p, channels);
  if (rc != CVH_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, CVH_ERR_HIP, "cvh_create: no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(nullptr, CVH_ERR_ARG, "cvh_create: device %d out of range [0,%d)", device, ndev);
  cvh_context *c = new (std::nothrow) cvh_context();
  if (!c) return fail(nullptr, CVH_ERR_NOMEM, "cvh_create: out of host memory");
  c->h = h; c->w = w; c->C = channels; c->device = device; c->n = (size_t)h * w; c->p = *p;
  rc = create_impl(c);
  if (rc != CVH_OK) {
    snprintf(g_create_err, kErrLen, "%s", c->err);
    cvh_destroy(c);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live.push_back(c);
  }
  *out = c;
  return CVH_OK;
}

extern "C" int cvh_set_params(cvh_context *c, const cvh_params *p)
{
  if (!c || !p) return CVH_ERR_ARG;
  int rc = check_params(c, p, c->C);
  if (rc != CVH_OK) return rc;
  if (p->eps != c->p.eps) c->sums_valid = false;
  c->p = *p;
  return CVH_OK;
}

extern "C" int cvh_set_option(cvh_context *c, const char *key, long value)
{
  if (!c || !key) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  { const int rc = settle(c); if (rc != CVH_OK) return rc; }  // options apply between runs
  { const int rc = one_buffer_leave(c); if (rc != CVH_OK) return rc; }   // and to the level set in d_u[] (the next enqueue chooses the flow again)
  if (!strcmp(key, "math_mode")) {
    if (value < 0 || value > 2) return fail(c, CVH_ERR_ARG, "math_mode must be 0, 1 or 2");
    c->math_mode = (int)value;
  } else if (!strcmp(key, "finalize")) {
    if (value != 0 && value != 1) return fail(c, CVH_ERR_ARG, "finalize must be 0 or 1");
    c->finalize_mode = (int)value;
  } else if (!strcmp(key, "tile_rows")) {
    if (value != 0 && value != 12 && value != 14 && value != 16) return fail(c, CVH_ERR_ARG, "tile_rows must be 0 (auto), 12, 14 or 16");
    c->tile_rows = (int)value;
  } else if (!strcmp(key, "kernel")) {
    if (value < -1 || value > 3 || value == 1)      // (1 was the strip kernel of round 1: never chosen, no fallback -- tools/experiments/pruned_flavours/)
      return fail(c, CVH_ERR_ARG, "kernel must be -1 (auto), 0 (tile), 2 (wave) or 3 (wave, 2 pixels per lane)");
    c->kernel = (int)value;
  } else if (!strcmp(key, "pm_kernel")) {
    if (value < -1 || value > 4 || value == 2)     // (2 was a 2-pixel-per-lane 1-step kernel: never chosen -- tools/experiments/pruned_flavours/)
      return fail(c, CVH_ERR_ARG, "pm_kernel must be -1 (auto), 0 (tile), 1 (wave), 3 (wave, 2 time steps per launch) or 4 (resident plane)");
    c->pm_kernel = (int)value;
  } else if (!strcmp(key, "res_straight")) {
    c->res_straight = value ? 1 : 0;
  } else if (!strcmp(key, "pm_strip_rows")) {
    if (value < 0) return fail(c, CVH_ERR_ARG, "pm_strip_rows must be >= 0");
    c->pm_strip_rows = (int)value;
  } else if (!strcmp(key, "wave_occupancy")) {
    if (value < 3 || value > 5) return fail(c, CVH_ERR_ARG, "wave_occupancy must be 3..5 (more waves per SIMD would spill registers)");
    c->wave_minw = (int)value;
  } else if (!strcmp(key, "debug_times")) {
    // diagnostic: per-wave start/end stamps of the wave kernel, read back with cvh_debug_read
    if (c->d_dbg) { HIPCHK(c, hipFree(c->d_dbg)); c->d_dbg = nullptr; c->dbg_words = 0; }
    if (value > 0) {
      c->dbg_words = (size_t)c->partial_rows * 20 + 16;
      if (c->dbg_words < (size_t)CVH_RESIDENT_MAX_TILES * 12 + 64) c->dbg_words = (size_t)CVH_RESIDENT_MAX_TILES * 12 + 64;   // resident kernel: 12 words per tile + 64 of the master
      HIPCHK(c, hipMalloc((void **)&c->d_dbg, c->dbg_words * 8));
      HIPCHK(c, hipMemset(c->d_dbg, 0, c->dbg_words * 8));
    }
  } else if (!strcmp(key, "graph")) {
    c->use_graph = value != 0;
  } else if (!strcmp(key, "wave_xcd")) {
    c->wave_xcd = value != 0;
  } else if (!strcmp(key, "wave_rev")) {
    c->wave_rev = value != 0;
  } else if (!strcmp(key, "wave_skew")) {
    if (value < 0 || value > 500) return fail(c, CVH_ERR_ARG, "wave_skew must be 0..500 (per mille)");
    c->wave_skew = (int)value;
  } else if (!strcmp(key, "chain")) {
    c->chain_opt = value != 0;
  } else if (!strcmp(key, "resident")) {
    if (value < -1 || value > 1) return fail(c, CVH_ERR_ARG, "resident must be -1 (auto), 0 or 1");
    c->resident_opt = (int)value;
  } else if (!strcmp(key, "far_terms")) {
    if (value != 4 && value != 5) return fail(c, CVH_ERR_ARG, "far_terms must be 4 or 5");
    c->far_terms = (int)value;
  } else if (!strcmp(key, "wave_pol")) {
    if (value < -1 || value > 2) return fail(c, CVH_ERR_ARG, "wave_pol must be -1 (auto), 0, 1 or 2 (diagnostic: non-temporal loads)");
    c->wave_pol = (int)value;
  } else if (!strcmp(key, "wave_cls")) {
    if (value < 0 || value > 2) return fail(c, CVH_ERR_ARG, "wave_cls must be 0 (off), 1 (2-pixel kernel) or 2 (1-pixel kernel too)");
    c->wave_cls = (int)value;
  } else if (!strcmp(key, "wave_cskew")) {
    if (value < 0 || value > 900) return fail(c, CVH_ERR_ARG, "wave_cskew must be 0..900 (per mille)");
    c->wave_cskew = (int)value;
  } else if (!strcmp(key, "wave_depth")) {
    if (value != 4 && value != 8) return fail(c, CVH_ERR_ARG, "wave_depth must be 4 or 8");
    c->wave_depth = (int)value;
  } else if (!strcmp(key, "wave_imgv")) {
    c->wave_imgv = value != 0;
  } else if (!strcmp(key, "wave_sync")) {
    c->wave_sync = value < 0 ? -1 : (value != 0);
  } else if (!strcmp(key, "wave_seam")) {
    if (value != 0 && value != 1) return fail(c, CVH_ERR_ARG, "wave_seam must be 0 or 1");
    c->wave_seam = (int)value;
  } else if (!strcmp(key, "one_buffer")) {
    if (value < -1 || value > 1) return fail(c, CVH_ERR_ARG, "one_buffer must be -1 (auto), 0 or 1");
    c->one_buffer = (int)value;
  } else if (!strcmp(key, "near_switch")) {
    c->near_switch = value != 0;
  } else if (!strcmp(key, "res_prio")) {
    c->res_prio = value != 0;
  } else if (!strcmp(key, "res_go_share")) {
    if (value < 0 || value > 6) return fail(c, CVH_ERR_ARG, "res_go_share must be 0 .. 6");
    c->res_go_share = (int)value;
  } else if (!strcmp(key, "co_resident")) {
    c->co_resident = value != 0;
  } else if (!strcmp(key, "state")) {
    // 64 (default): the level set lives in HBM as double, the reference's CV_64FC1 (src/main.cpp:225) -- the parity mode.
    // 32: DECLARED fast mode -- float in HBM (9 instead of 17 bytes per pixel-iteration), arithmetic and sums unchanged; every new value is
    // rounded to float.  2-pixel wave kernel only (FAST arithmetic, width a multiple of 16 and >= 144, < 2^28 pixels).
    if (value != 32 && value != 64) return fail(c, CVH_ERR_ARG, "state must be 64 or 32");
    if ((int)value != c->state_bits) {
      if (value == 32) {
        if (c->w % 16 != 0 || c->w < 144 || c->n >= ((size_t)1 << 28))
          return fail(c, CVH_ERR_ARG, "state 32 needs a width that is a multiple of 16 and >= 144, and fewer than 2^28 pixels (the 2-pixel wave kernel)");
        c->state_bits = 32;
        if (c->have_u) { const int rc = adopt_f32_state(c); if (rc != CVH_OK) return rc; }
      } else {
        if (c->have_u) { const int rc = ensure_f64_mirror(c); if (rc != CVH_OK) return rc; }
        c->state_bits = 64;
        c->mirror_valid = true;
      }
      c->sums_valid = false;
    }
  } else if (!strcmp(key, "wave_prio")) {
    if (value < 0 || value > 4) return fail(c, CVH_ERR_ARG, "wave_prio must be 0..4");
    c->wave_prio = (int)value;
  } else if (!strcmp(key, "wave_lds_cap")) {
    c->wave_lds_cap = value != 0;
  } else if (!strcmp(key, "strip_rows")) {
    if (value < 0) return fail(c, CVH_ERR_ARG, "strip_rows must be >= 0");
    c->strip_rows = (int)value;
  } else if (!strcmp(key, "strips")) {
    if (value < 0 || value > c->h) return fail(c, CVH_ERR_ARG, "strips must be 0 (auto) .. h");
    c->strips = (int)value;
  } else if (!strcmp(key, "lut")) {
    c->use_lut = value != 0;
  } else if (!strcmp(key, "dma")) {
    c->use_dma = value != 0;
  } else if (!strcmp(key, "sync_every")) {
    if (value < 1) return fail(c, CVH_ERR_ARG, "sync_every must be >= 1");
    c->sync_every = (int)(value > 1000000 ? 1000000 : value);
  } else if (!strcmp(key, "trace")) {
    if (value < 0) return fail(c, CVH_ERR_ARG, "trace capacity must be >= 0");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->d_trace) { HIPCHK(c, hipFree(c->d_trace)); c->d_trace = nullptr; }
    c->trace_cap = 0;
    if (value > 0) {
      const size_t bytes = (size_t)value * (2 * c->C + 1) * sizeof(double);
      HIPCHK(c, hipMalloc((void **)&c->d_trace, bytes));
      HIPCHK(c, hipMemset(c->d_trace, 0, bytes));
      c->trace_cap = (int)value;
    }
  } else {
    return fail(c, CVH_ERR_ARG, "unknown option \"%s\"", key);
  }
  return CVH_OK;
}

// tol-free part of the stop condition, src/main.cpp:950-959 (zero-initialised accumulator, channels added serially in k,
// scaled by 1/C, L2 norm with four squares per step added left to right).  (sum_k I_k)/C squared takes one of 255 C + 1
// values: the table keeps the reference's rounding and summation order while the loop is integer adds and lookups.
double stop_norm_host(const std::vector<const uint8_t *> &planes, size_t n)
{
  const int C = (int)planes.size();
  const double inv = 1.0 / C;
  double sq[CVH_MAX_CHANNELS * 255 + 1];
  for (int t = 0; t <= 255 * C; ++t) { const double v = (double)t * inv; sq[t] = v * v; }
  auto at = [&](size_t q) {
    int t = 0;
    for (int k = 0; k < C; ++k) t += planes[k][q];
    return sq[t];
  };
  double s = 0;
  size_t i = 0;
  for (; i + 4 <= n; i += 4) s += ((at(i) + at(i + 1)) + at(i + 2)) + at(i + 3);
  for (; i < n; ++i) s += at(i);
  return sqrt(s);
}

// Sums of the planes resident on the device: sum(I_k) for the region means and, for one channel, the stop norm (exact
// integers, image_sums_kernel in io_kernels.hip).  Three channels round (sum_k I_k)/3 per pixel, so their norm needs the reference's serial
// order: `host_planes` (the caller's buffers, or nullptr to fetch the planes) feed stop_norm_host.
int image_stats(cvh_context *c, const uint8_t *const *host_planes)
{
  HIPCHK(c, hipMemsetAsync(c->d_isums, 0, 8 * sizeof(unsigned long long), c->stream));
  HIPCHK(c, cvh_launch_image_sums(c->d_img, c->C, c->n, c->d_isums, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->h_isums, c->d_isums, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  const bool exact_on_device = stop_norm_exact_on_device(c);
  std::vector<std::vector<uint8_t>> fetched;
  std::vector<const uint8_t *> pl;
  if (!exact_on_device) {
    if (host_planes) pl.assign(host_planes, host_planes + c->C);
    else {
      try { fetched.assign(c->C, std::vector<uint8_t>(c->n)); } catch (...) { return fail(c, CVH_ERR_NOMEM, "out of host memory"); }
      for (int k = 0; k < c->C; ++k) {
        HIPCHK(c, hipMemcpyAsync(fetched[k].data(), c->d_img[k], c->n, hipMemcpyDeviceToHost, c->stream));
        pl.push_back(fetched[k].data());
      }
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double host_norm = exact_on_device ? 0.0 : stop_norm_host(pl, c->n);
  plane_sums_arrived(c, c->h_isums, exact_on_device ? nullptr : &host_norm);
  return CVH_OK;
}

extern "C" int cvh_set_image(cvh_context *c, const uint8_t *const *planes)
{
  if (!c || !planes) return CVH_ERR_ARG;
  for (int k = 0; k < c->C; ++k) if (!planes[k]) return fail(c, CVH_ERR_ARG, "cvh_set_image: plane %d is NULL", k);
  HIPCHK(c, hipSetDevice(c->device));
  { const int rc = settle(c); if (rc != CVH_OK) return rc; }
  for (int k = 0; k < c->C; ++k)
    HIPCHK(c, hipMemcpyAsync(c->d_img[k], planes[k], c->n, hipMemcpyHostToDevice, c->stream));
  return image_stats(c, planes);
}

extern "C" int cvh_get_image(cvh_context *c, uint8_t *const *planes)
{
  if (!c || !planes) return CVH_ERR_ARG;
  if (!c->have_image) return fail(c, CVH_ERR_STATE, "cvh_get_image: no image set");
  HIPCHK(c, hipSetDevice(c->device));
  for (int k = 0; k < c->C; ++k) {
    if (!planes[k]) return fail(c, CVH_ERR_ARG, "cvh_get_image: plane %d is NULL", k);
    HIPCHK(c, hipMemcpyAsync(planes[k], c->d_img[k], c->n, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CVH_OK;
}

// ---- The transitions of a context's run state (the group of that name in cvh_context, cvh_host.h): what the context has in flight and
// which of its cached values are still true.  Every flow calls these instead of assigning the fields; each function states the invariant
// it keeps.  sync_impl (csv_run.hip), which closes what these open, is the one other place that assigns them. ----
// Work in flight is settled: iterations enqueued and never synchronised (chain_pending) or a timed interval that is still open are closed
// before a caller replaces state they read -- options, planes, the level set, the shared CvhResident block.  No third term: a resident
// launch (resident_used) is enqueued by cvh_enqueue_steps, which has opened the interval by then, or by cvh_run, which ends in sync_impl, and
// sync_impl alone closes the interval -- together with resident_used.  So resident_used implies timing_open wherever every earlier call
// succeeded (the Perona-Malik callers used to test it as well; it could add nothing there).
int settle(cvh_context *c) { return c->timing_open || c->chain_pending ? sync_impl(c) : CVH_OK; }

// A new run begins, host half: counter and stop flag cleared, the automatic choices of a run are taken again (live-context registry).  The
// buffer holding u becomes the base, and so does the chain-mode sum set that belongs to it.
static void begin_run_host(cvh_context *c)
{
  c->cur_base = current_buffer(c);
  c->chain_pb = (c->chain_pb + c->steps_done) & 3;
  c->steps_done = 0;
  c->enqueued = 0;
  c->run_pol = -1; c->run_alone = -1; c->run_chunk = -1;
  c->h_status[0] = 0; c->h_status[1] = 0;
}

// A new run begins, device half, enqueued on s: the state block's counters and the sum set after the run's own (it may hold the sums of an
// iteration computed past a stop) are cleared.  The ONE place that says what that is for the host (the kernels that write a level set do
// the same through CvhIoMember's state_zero / chain_zero).
hipError_t clear_run_device(cvh_context *c, hipStream_t s)
{
  static const int zeros[4] = {0, 0, 0, 0};   // steps_done, stopped, ticket, pending
  const hipError_t e = hipMemcpyAsync(&c->d_state->steps_done, zeros, sizeof(zeros), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return e;
  return hipMemsetAsync(&c->d_chain->v[(c->chain_pb + 1) & 3][0], 0, sizeof(c->d_chain->v[0]), s);
}

// A new run begins: whatever is in flight is settled, then the host half, then the device half, and the host waits for that.
int reset_run_impl(cvh_context *c)
{
  { const int rc = settle(c); if (rc != CVH_OK) return rc; }
  begin_run_host(c);
  HIPCHK(c, clear_run_device(c, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CVH_OK;
}

// A level set has arrived in d_u[chain_pb & 1], and the copy or launch that brought it has completed: only now does the bookkeeping follow
// the data.  The buffer is the one whose parity equals the chain-mode sum set's: the ping-pong parity and the sum-set phase of a launch
// then stay locked together (cur_base == chain_pb mod 2), and a cached step graph of a phase is valid for every run.  FP32 state takes the
// level set over; then the new run -- its host half alone where the launch that wrote the level set did the device half (device_cleared).
int levelset_arrived(cvh_context *c, bool device_cleared)
{
  c->cur_base = c->chain_pb & 1; c->steps_done = 0; c->enqueued = 0;
  c->have_u = true;
  c->sums_valid = false;
  c->mirror_valid = true;
  c->ob_live = false;            // (the one-buffer slab held the level set this one replaces)
  if (c->state_bits == 32) { const int rc = adopt_f32_state(c); if (rc != CVH_OK) return rc; }
  if (!device_cleared) return reset_run_impl(c);
  begin_run_host(c);
  return CVH_OK;
}

// n > 0 steps were really enqueued (never called while capturing) on a grid of nparts workgroups.  Chain mode: the last of them has no
// successor to book it yet -- the next launch on the same grid does, or the flush kernel, which also writes c1 / c2 of the final level set
// into the state block at the next sync; otherwise the means now live in the state block only.  pending_nparts is 0 for a resident launch,
// which books its iterations itself and leaves its error word for sync_impl.  FP32 state: the double mirror is behind.
void steps_enqueued(cvh_context *c, int n, int nparts, bool chain, bool resident)
{
  if (resident) { nparts = 0; c->resident_used = true; }
  if (chain) { c->chain_pending = true; c->pending_nparts = nparts; }
  else c->chain_acc_valid = false;
  c->last_nparts = nparts;
  if (c->state_bits == 32 || c->ob_live) c->mirror_valid = false;
  c->enqueued += n;
}

// The initial sums of the current level set were taken: c1 / c2 are in the state block and, in chain mode, the fixed-point set is seeded.
void sums_taken(cvh_context *c, bool chain) { c->sums_valid = true; c->chain_acc_valid = chain; }

// One channel and fewer than 2^36 pixels: the stop norm is exact on the device (integers, 2^36 * 255^2 < 2^53).  Three channels round
// (sum_k I_k)/3 per pixel, so their norm needs the reference's serial order on the host (stop_norm_host).
bool stop_norm_exact_on_device(const cvh_context *c) { return c->C == 1 && c->n < ((size_t)1 << 36); }

// The planes changed on the device (an upload or ingest replaced them, Perona-Malik smoothed them): the region means were taken against
// the old planes, and the stop norm is theirs until plane sums come back.
void planes_changed(cvh_context *c) { c->stop_valid = false; c->sums_valid = false; }

// Plane sums have come back: isums holds {sum p, sum p^2} per plane (exact integers: < 2^53 as doubles), host_norm the norm the host took
// where the device's is not exact (else nullptr).  The context holds an image whose stop norm is valid and whose means are not.
void plane_sums_arrived(cvh_context *c, const unsigned long long *isums, const double *host_norm)
{
  planes_changed(c);
  for (int k = 0; k < c->C; ++k) c->sum_img[k] = (double)isums[2 * k];
  c->stop_norm = host_norm ? *host_norm : sqrt((double)isums[1]);
  c->stop_valid = true;
  c->have_image = true;
}

// FP32 state: the float buffers (lazily allocated) take over the level set that d_u[current] holds -- rounded to float, and d_u[current]
// is rewritten with the rounded values, so that whatever reads the mirror (initial sums, mask, get) sees what the kernels iterate on.
int adopt_f32_state(cvh_context *c)
{
  if (!c->d_uf_slab) {
    const size_t each = (((c->n + 64) * sizeof(float)) + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    HIPCHK(c, hipMalloc((void **)&c->d_uf_slab, 2 * each));
    c->d_uf[0] = (float *)c->d_uf_slab;
    c->d_uf[1] = (float *)((char *)c->d_uf_slab + each);
  }
  const int cur = current_buffer(c);
  HIPCHK(c, cvh_launch_state_narrow(c->d_u[cur], c->d_uf[cur], c->n, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->mirror_valid = true;
  c->sums_valid = false;
  return CVH_OK;
}

// FP32 state: d_u[current] = (double) d_uf[current] if launches have run since the mirror was last refreshed (call behind a sync).
// One-buffer flow: d_u[current] = the plane rows of the slab, likewise.
int ensure_f64_mirror(cvh_context *c)
{
  if ((c->state_bits != 32 && !c->ob_live) || c->mirror_valid) return CVH_OK;
  { const int rc = settle(c); if (rc != CVH_OK) return rc; }
  const int cur = current_buffer(c);
  if (c->ob_live) {
    HIPCHK(c, cvh_launch_ob_unpack(c->d_ob, c->d_u[cur], c->h, c->w, (c->w + cvh_wave2_cols() - 1) / cvh_wave2_cols(), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mirror_valid = true;
    return CVH_OK;
  }
  HIPCHK(c, cvh_launch_state_widen(c->d_uf[cur], c->d_u[cur], c->n, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->mirror_valid = true;
  return CVH_OK;
}

extern "C" int cvh_reset_run(cvh_context *c)
{
  if (!c) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  return reset_run_impl(c);
}

extern "C" int cvh_set_levelset(cvh_context *c, const double *u)
{
  if (!c || !u) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  { const int rc = settle(c); if (rc != CVH_OK) return rc; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_u[c->chain_pb & 1], u, c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return levelset_arrived(c);
}

// src/main.cpp:226-231: the factors of sign(sin(pi*i/5) * sin(pi*j/5)), host libm, double -- the h row factors, then the w column factors.
// The ONE place they are computed: the host form below and the device form (checkerboard_batch, io_run.hip) multiply the same doubles.
void checkerboard_factors(int h, int w, double *out)
{
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < h; ++i) out[i] = sin(pi * i / 5);
  for (int j = 0; j < w; ++j) out[(size_t)h + j] = sin(pi * j / 5);
}

extern "C" void cvh_levelset_checkerboard_host(int h, int w, double *u)
{
  std::vector<double> sv((size_t)h + w);
  checkerboard_factors(h, w, sv.data());
  for (int i = 0; i < h; ++i)
    for (int j = 0; j < w; ++j) {
      const double z = sv[i] * sv[(size_t)h + j];
      u[(size_t)i * w + j] = (z == 0) ? 0.0 : (z < 0 ? -1.0 : 1.0);
    }
}

extern "C" int cvh_get_levelset(cvh_context *c, double *u)
{
  if (!c || !u) return CVH_ERR_ARG;
  if (!c->have_u) return fail(c, CVH_ERR_STATE, "cvh_get_levelset: no level set");
  HIPCHK(c, hipSetDevice(c->device));
  { const int rc = ensure_f64_mirror(c); if (rc != CVH_OK) return rc; }
  HIPCHK(c, hipMemcpyAsync(u, c->d_u[current_buffer(c)], c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CVH_OK;
}

extern "C" int cvh_get_means(cvh_context *c, double *c1, double *c2)
{
  if (!c || !c1 || !c2) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->timing_open) return fail(c, CVH_ERR_STATE, "cvh_get_means: steps in flight, call cvh_sync first");
  int rc = prepare(c);
  if (rc != CVH_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(&c->h_state[0], c->d_state, sizeof(CvhState), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < c->C; ++k) { c1[k] = c->h_state[0].c1[k]; c2[k] = c->h_state[0].c2[k]; }
  return CVH_OK;
}

extern "C" int cvh_get_trace(cvh_context *c, double *out, int max_rows, int *rows)
{
  if (!c || !out || !rows || max_rows < 0) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int n = c->steps_done < c->trace_cap ? c->steps_done : c->trace_cap;
  if (n > max_rows) n = max_rows;
  *rows = n;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(out, c->d_trace, (size_t)n * (2 * c->C + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return CVH_OK;
}

extern "C" int cvh_get_stop_condition(cvh_context *c, double *stop_cond)
{
  if (!c || !stop_cond) return CVH_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc = prepare(c);
  if (rc != CVH_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *stop_cond = c->p.tol * c->stop_norm;
  return CVH_OK;
}

extern "C" int cvh_get_mask(cvh_context *c, uint8_t *mask, int invert)
{
  if (!c || !mask) return CVH_ERR_ARG;
  if (!c->have_u) return fail(c, CVH_ERR_STATE, "cvh_get_mask: no level set");
  static const char what[] = "cvh_get_mask";   // a mask batch of one into the context's own buffer: iterations in flight are settled first
  return mask_to_host(c, mask, [&]() { return mask_out(&c, 1, &c->d_mask, invert, c->stream, what); });
}

extern "C" int cvh_get_contour(cvh_context *c, uint8_t *contour)
{
  if (!c || !contour) return CVH_ERR_ARG;
  if (!c->have_u) return fail(c, CVH_ERR_STATE, "cvh_get_contour: no level set");
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->d_mask) HIPCHK(c, hipMalloc((void **)&c->d_mask, c->n));
  { const int rc = ensure_f64_mirror(c); if (rc != CVH_OK) return rc; }
  HIPCHK(c, cvh_launch_contour(c->d_u[current_buffer(c)], c->d_mask, c->h, c->w, c->stream));
  HIPCHK(c, hipMemcpyAsync(contour, c->d_mask, c->n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return CVH_OK;
}

extern "C" int cvh_separate(cvh_context *c, const uint8_t *img3, int invert, uint8_t *selection3)
{
  if (!c || !img3 || !selection3) return CVH_ERR_ARG;
  if (!c->have_u) return fail(c, CVH_ERR_STATE, "cvh_separate: no level set");
  HIPCHK(c, hipSetDevice(c->device));
  { const int rc = ensure_f64_mirror(c); if (rc != CVH_OK) return rc; }
  uint8_t *d_in = nullptr, *d_out = nullptr;
  HIPCHK(c, hipMalloc((void **)&d_in, c->n * 3));
  hipError_t e = hipMalloc((void **)&d_out, c->n * 3);
  if (e != hipSuccess) { (void)hipFree(d_in); return fail(c, CVH_ERR_HIP, "hipMalloc: %s", hipGetErrorString(e)); }
  int rc = CVH_OK;
  do {
    if ((e = hipMemcpyAsync(d_in, img3, c->n * 3, hipMemcpyHostToDevice, c->stream)) != hipSuccess) break;
    if ((e = cvh_launch_separate(d_in, c->d_u[current_buffer(c)], d_out, c->n, invert, c->stream)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(selection3, d_out, c->n * 3, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
    e = hipStreamSynchronize(c->stream);
  } while (0);
  if (e != hipSuccess) rc = fail(c, CVH_ERR_HIP, "cvh_separate: %s", hipGetErrorString(e));
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return rc;
}

extern "C" int cvh_last_run_ms(cvh_context *c, float *ms)
{
  if (!c || !ms) return CVH_ERR_ARG;
  *ms = c->last_run_ms;
  return CVH_OK;
}

extern "C" int cvh_last_pm_ms(cvh_context *c, float *ms)
{
  if (!c || !ms) return CVH_ERR_ARG;
  *ms = c->last_pm_ms;
  return CVH_OK;
}

extern "C" int cvh_ppf_apply_device(double *d_data, long n, int op, double eps, void *stream)
{
  if (!d_data || n < 0 || op < 0 || op > 2) return fail(nullptr, CVH_ERR_ARG, "cvh_ppf_apply_device: bad argument");
  hipError_t e = cvh_launch_ppf(d_data, (size_t)n, op, eps, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, CVH_ERR_HIP, "cvh_ppf_apply_device: %s", hipGetErrorString(e));
  return CVH_OK;
}

extern "C" int cvh_ppf_apply(double *data, int w, long start, long end, int op, double eps, int device)
{
  // data.at<double>(i / w, i % w) of a continuous w-wide matrix is data[i]
  if (!data || w <= 0 || start < 0 || end < start || op < 0 || op > 2)
    return fail(nullptr, CVH_ERR_ARG, "cvh_ppf_apply: bad argument");
  if (end == start) return CVH_OK;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(nullptr, CVH_ERR_HIP, "cvh_ppf_apply: hipSetDevice: %s (no CPU fallback)", hipGetErrorString(e));
  const size_t n = (size_t)(end - start);
  // OpenCV's backend calls the operator once per sub-range from several host threads: the staging buffer comes from the
  // device's stream-ordered memory pool (cached between calls; no device-wide synchronisation as with hipMalloc / hipFree)
  // and everything runs on a stream of its own, so concurrent sub-ranges do not serialise on the null stream.
  hipStream_t st = nullptr;
  if ((e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess)
    return fail(nullptr, CVH_ERR_HIP, "cvh_ppf_apply: hipStreamCreate: %s", hipGetErrorString(e));
  double *d = nullptr;
  bool pooled = true;
  if (hipMallocAsync((void **)&d, n * sizeof(double), st) != hipSuccess) {
    (void)hipGetLastError();
    pooled = false;
    if ((e = hipMalloc((void **)&d, n * sizeof(double))) != hipSuccess) {
      (void)hipStreamDestroy(st);
      return fail(nullptr, CVH_ERR_HIP, "cvh_ppf_apply: hipMalloc: %s", hipGetErrorString(e));
    }
  }
  do {
    if ((e = hipMemcpyAsync(d, data + start, n * sizeof(double), hipMemcpyHostToDevice, st)) != hipSuccess) break;
    if ((e = cvh_launch_ppf(d, n, op, eps, st)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(data + start, d, n * sizeof(double), hipMemcpyDeviceToHost, st)) != hipSuccess) break;
    e = hipStreamSynchronize(st);
  } while (0);
  if (pooled) { (void)hipFreeAsync(d, st); (void)hipStreamSynchronize(st); } else (void)hipFree(d);
  (void)hipStreamDestroy(st);
  if (e != hipSuccess) return fail(nullptr, CVH_ERR_HIP, "cvh_ppf_apply: %s", hipGetErrorString(e));
  return CVH_OK;
}

extern "C" int cvh_launch_info(cvh_context *c, int phase, char *buf, int cap)
{
  if (!c || !buf || cap < 1 || (phase != 0 && phase != 1)) return CVH_ERR_ARG;
  if (phase == 1) {
    if (!c->pm_desc[0]) return fail(c, CVH_ERR_STATE, "cvh_launch_info: cvh_perona_malik has not run on this context");
    snprintf(buf, (size_t)cap, "%s", c->pm_desc);
    return CVH_OK;
  }
  // the CSV step as the next cvh_run / cvh_enqueue_steps would launch it: the launcher itself describes it (CVH_LAUNCH)
  CvhLaunchNote note{};
  {
    ResidentGeom rg;
    if (resident_geometry(c, &rg)) {
      const int rc = launch_resident(c, rg, 1, &note);
      if (rc != CVH_OK) return rc;
      snprintf(buf, (size_t)cap, "kernel=%s grid=%u block=%u lds_bytes=%u data_flow=4 tiles_y=%d tiles_x=%d tile_rows=%d chain=1 math=fast "
               "steps_per_launch=chunk", note.name, note.grid, note.block, note.lds, rg.tr, rg.tc, (c->h + rg.tr - 1) / rg.tr);
      return CVH_OK;
    }
  }
  const int rc = launch_one_step(c, current_buffer(c), c->enqueued, true, &note);
  if (rc != CVH_OK) return rc;
  const Geometry g = resolve_geometry(c);
  CvhStepArgs a;
  fill_args(c, &a, current_buffer(c), c->enqueued);
  snprintf(buf, (size_t)cap, "kernel=%s grid=%u block=%u lds_bytes=%u data_flow=%d wave_columns=%d strips=%d strip_rows=%d chain=%d "
           "wave_pol=%d math=%s steps_per_graph=%d wave_seam=%d one_buffer=%d", note.name, note.grid, note.block, note.lds, g.strip, g.tiles_x, g.tiles_y,
           g.strip_rows, a.chain ? 1 : 0, a.wave_pol, use_fast(c) ? "fast" : "strict", c->use_graph ? kGraphSteps : 0,
           (g.strip == 3 && use_fast(c)) ? a.wave_seam : 0, a.one_buffer);
  return CVH_OK;
}

