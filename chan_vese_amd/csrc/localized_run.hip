// localized_run.hip — host side of the localised-regions calls (include/chanvese_hip.h, "Localised regions"; kernels in
// localized_kernels.hip).  A call checks everything, settles the context as the getters do and takes the planes T_k once;
// cvh_localized_run then hands the iterations to march_run.hip's driver: three launches per iteration on the context's stream -- row
// pass, step, finalise.
// The workspace, kept by the context: [state block][the items' partial sums][1 + C planes of 8 bytes: the horizontal window sums][C
// planes of 4 bytes: T_k] -- 8 + 12 C bytes per pixel, whatever the radius.
#include "cvh_host.h"

namespace {

constexpr size_t kLocStateBytes = 256;
static_assert(sizeof(CvhLocState) <= kLocStateBytes, "the workspace's first section holds the state block");
static_assert(sizeof(CvhLocState) <= 4 * sizeof(CvhState), "the state block comes down into the context's pinned state slots");

// What every call refuses before anything is touched
int loc_check(cvh_context *c, int radius, const char *what)
{
  cvh_context *ctxs[1] = {c};
  if (radius < 1 || radius > CVH_LOC_RADIUS_MAX)
    return batch_fail(ctxs, 1, CVH_ERR_ARG, "%s: radius = %d, must be 1 .. %d", what, radius, CVH_LOC_RADIUS_MAX);
  if (c->state_bits == 32) return batch_fail(ctxs, 1, CVH_ERR_ARG, "%s: the context has \"state\" = 32: the call iterates an FP64 level set", what);
  if (c->n >= ((size_t)1 << 28)) return batch_fail(ctxs, 1, CVH_ERR_ARG, "%s: %d x %d is too large, h * w must stay below 2^28", what, c->h, c->w);
  if (!c->have_image) return batch_fail(ctxs, 1, CVH_ERR_STATE, "%s: the context has no image (call cvh_set_image first)", what);
  if (!c->have_u) return batch_fail(ctxs, 1, CVH_ERR_STATE, "%s: the context has no level set", what);
  return CVH_OK;
}

size_t partial_bytes(const CvhLocGeom &g) { return align_up((size_t)g.nitems * sizeof(double), 256); }

// the context settled, its FP64 mirror fresh, the workspace there
int loc_ready(cvh_context *c, const char *what, const CvhLocGeom &g)
{
  cvh_context *ctxs[1] = {c};
  HIPCHK(c, hipSetDevice(c->device));
  int rc = settle_all(ctxs, 1, what);
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(ctxs, 1, what);
  if (rc != CVH_OK) return rc;
  const size_t bytes = kLocStateBytes + partial_bytes(g) + c->n * ((1 + c->C) * sizeof(unsigned long long) + c->C * sizeof(unsigned));
  const bool fresh = !c->d_localized;
  rc = ensure_workspace(c, &c->d_localized, bytes, "localised-regions", false);
  if (rc != CVH_OK) return batch_fail(ctxs, 1, rc, "%s: %s", what, c->err);
  if (fresh) HIPCHK(c, hipMemsetAsync(c->d_localized, 0, kLocStateBytes, c->stream));   // a state block never holds what hipMalloc left there
  return CVH_OK;
}

// everything of the launch arguments but in / out, the trace and the planes of cvh_localized_means
void loc_args(const cvh_context *c, int radius, const CvhLocGeom &g, CvhLocArgs *m)
{
  memset(m, 0, sizeof(*m));
  for (int k = 0; k < c->C; ++k) m->img[k] = c->d_img[k];
  unsigned char *ws = (unsigned char *)c->d_localized;
  m->st = (CvhLocState *)ws;
  m->partials = (double *)(ws + kLocStateBytes);
  m->hw = (unsigned long long *)(ws + kLocStateBytes + partial_bytes(g));
  m->tsum = (unsigned *)(m->hw + (size_t)(1 + c->C) * c->n);
  m->h = c->h; m->w = c->w; m->radius = radius;
  m->g = g;
  m->alpha = c->p.mu * c->p.dt;          // the folded combine, as fill_args (csv_run.hip)
  m->beta = (1.0 / c->C) * c->p.dt;
  m->gamma = -c->p.nu * c->p.dt;
  for (int k = 0; k < c->C; ++k) { m->lambda1[k] = c->p.lambda1[k]; m->lambda2[k] = c->p.lambda2[k]; }
  m->stop = c->p.tol * c->stop_norm;
  fill_front_args(c, &m->f);
}

// T_k, once per call: a row pass with wq = 1 and the wave kernel's vertical sums of it
int plane_sums(cvh_context *c, const CvhLocArgs &m)
{
  HIPCHK(c, cvh_launch_loc_rows(m, c->C, 0, CVH_LOC_TSUM, c->stream));
  HIPCHK(c, cvh_launch_loc_wave(m, c->C, 0, CVH_LOC_TSUM, c->stream));
  return CVH_OK;
}

int localized_run(cvh_context *c, int radius, int max_steps, int *steps_done, double *norm, double *trace, int trace_rows, int *rows,
                  const char *what)
{
  cvh_context *ctxs[1] = {c};
  int rc = loc_check(c, radius, what);
  if (rc != CVH_OK) return rc;
  MarchRun run{ctxs, 1, what, ""};
  rc = run.begin(max_steps, trace, trace_rows, rows);
  if (rc != CVH_OK) return rc;
  const CvhLocGeom g = cvh_loc_geometry(c->h, c->w, radius);
  rc = loc_ready(c, what, g);
  if (rc != CVH_OK) return rc;
  rc = prepare_host(c);   // the stop norm (taken again where the planes changed on the device)
  if (rc != CVH_OK) return batch_fail(ctxs, 1, rc, "%s: %s", what, c->err);
  const int C = c->C, fast = use_fast(c);
  rc = run.open(&c->loc_trace, 1);
  if (rc != CVH_OK) return rc;
  CvhLocArgs m;
  loc_args(c, radius, g, &m);
  m.trace = run.d_trace; m.trace_cap = run.trace_cap;
  // no launch in front of the first iteration writes the state block (the four-phase flow's initial finalise does): zeroed here
  HIPCHK(c, hipMemsetAsync(c->d_localized, 0, kLocStateBytes, c->stream));
  rc = plane_sums(c, m);
  if (rc != CVH_OK) return rc;
  CvhLocState st;
  rc = run.iterate(c->d_localized, &st, sizeof(st), [&](const double *const *in, double *const *out) -> int {
    m.in = in[0]; m.out = out[0];
    HIPCHK(c, cvh_launch_loc_rows(m, C, fast, CVH_LOC_STEP, c->stream));
    HIPCHK(c, cvh_launch_loc_wave(m, C, fast, CVH_LOC_STEP, c->stream));
    HIPCHK(c, cvh_launch_loc_finalize(m, c->stream));
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  if (steps_done) *steps_done = st.run.steps_done;
  if (norm) *norm = st.norm;
  return CVH_OK;
}

int localized_means(cvh_context *c, int radius, double *c1, double *c2, uint64_t *wq, uint64_t *a, uint64_t *s, const char *what)
{
  cvh_context *ctxs[1] = {c};
  int rc = loc_check(c, radius, what);
  if (rc != CVH_OK) return rc;
  if (!c1 && !c2 && !wq && !a && !s) return batch_fail(ctxs, 1, CVH_ERR_ARG, "%s: every output is NULL", what);
  const CvhLocGeom g = cvh_loc_geometry(c->h, c->w, radius);
  rc = loc_ready(c, what, g);
  if (rc != CVH_OK) return rc;
  CvhLocArgs m;
  loc_args(c, radius, g, &m);
  // the asked planes, on the device for the length of the call: [c1][c2][wq][a][s], 8 bytes an entry
  void *const host[5] = {c1, c2, wq, a, s};
  const size_t planes[5] = {(size_t)c->C, (size_t)c->C, 1, 1, (size_t)c->C};
  size_t off[5], total = 0;
  for (int i = 0; i < 5; ++i) { off[i] = total; if (host[i]) total += planes[i] * c->n * 8; }
  unsigned char *d = nullptr;
  const hipError_t e = hipMalloc((void **)&d, total);
  if (e != hipSuccess) return batch_fail(ctxs, 1, CVH_ERR_HIP, "%s: hipMalloc of %zu bytes for the planes: %s", what, total, hipGetErrorString(e));
  if (c1) m.c1_out = (double *)(d + off[0]);
  if (c2) m.c2_out = (double *)(d + off[1]);
  if (wq) m.wq_out = (unsigned long long *)(d + off[2]);
  if (a) m.a_out = (unsigned long long *)(d + off[3]);
  if (s) m.s_out = (unsigned long long *)(d + off[4]);
  m.in = c->d_u[current_buffer(c)];
  auto body = [&]() -> int {
    int r2 = open_call(ctxs, 1, nullptr);
    if (r2 != CVH_OK) return r2;
    r2 = plane_sums(c, m);
    if (r2 != CVH_OK) return r2;
    HIPCHK(c, cvh_launch_loc_rows(m, c->C, use_fast(c), CVH_LOC_MEANS, c->stream));
    HIPCHK(c, cvh_launch_loc_wave(m, c->C, 0, CVH_LOC_MEANS, c->stream));
    for (int i = 0; i < 5; ++i)
      if (host[i]) HIPCHK(c, hipMemcpyAsync(host[i], d + off[i], planes[i] * c->n * 8, hipMemcpyDeviceToHost, c->stream));
    r2 = close_call(ctxs, 1, nullptr, false);
    if (r2 != CVH_OK) return r2;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CVH_OK;
  };
  rc = body();
  (void)hipFree(d);   // (waits for the device)
  return rc;
}

}  // namespace

extern "C" int cvh_localized_run(cvh_context *ctx, int radius, int max_steps, int *steps_done, double *norm, double *trace, int trace_rows,
                                 int *rows)
{
  return guarded_one(ctx, "cvh_localized_run",
                     [&](const char *what) { return localized_run(ctx, radius, max_steps, steps_done, norm, trace, trace_rows, rows, what); });
}

extern "C" int cvh_localized_means(cvh_context *ctx, int radius, double *c1, double *c2, uint64_t *wq, uint64_t *a, uint64_t *s)
{
  return guarded_one(ctx, "cvh_localized_means", [&](const char *what) { return localized_means(ctx, radius, c1, c2, wq, a, s, what); });
}

extern "C" void cvh_localized_geometry(int h, int w, int radius, int *cols, int *item_rows, int *items, int *strip_rows)
{
  CvhLocGeom g;
  memset(&g, 0, sizeof(g));
  if (h > 0 && w > 0 && (long long)h * w < (1ll << 28) && radius >= 1 && radius <= CVH_LOC_RADIUS_MAX) g = cvh_loc_geometry(h, w, radius);
  if (cols) *cols = CVH_MARCH_COLS;
  if (item_rows) *item_rows = g.item_rows;
  if (items) *items = g.nitems;
  if (strip_rows) *strip_rows = g.strip_rows;
}
