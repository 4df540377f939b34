// localized_run.hip — host side of the localised-regions calls (include/chanvese_hip.h, "Localised regions"; kernels in
// localized_kernels.hip).  A call checks everything, settles its members as the getters do and takes the planes T_k once;
// cvh_localized_run_batch then hands the iterations to march_run.hip's driver: per iteration and (channel count, math mode) class three
// launches on the leader's stream -- row pass, step, finalise -- over the members of that class.  cvh_localized_run is the batch of one
// member and cvh_localized_means takes the same launches: one host path.  A call with ONE member keeps the single call's launches as
// they were before the batch existed: the record by value (the kernel bodies' second entry point), no upload, no mirror, the host reads
// the member's own state block (DESIGN.md 4.17b says what the table form cost a single plane).
// The workspace, kept by each context: [state block][the items' partial sums][1 + C planes of 8 bytes: the horizontal window sums][C
// planes of 4 bytes: T_k] -- 8 + 12 C bytes per pixel, whatever the radius.  The table of a call -- the members' argument records and
// their state slots -- is the leader's (MarchRun).
#include "cvh_host.h"

namespace {

constexpr size_t kLocStateBytes = 256;
constexpr size_t kLocSlotBytes = 64;   // a member's slot of the leader's state table
static_assert(sizeof(CvhLocState) <= kLocStateBytes, "the workspace's first section holds the state block");
static_assert(sizeof(CvhLocState) <= kLocSlotBytes, "a slot of the state table holds the state block");

// What every call refuses for a member before anything is touched; `who` opens what the message says ("" or "member 3: ")
int loc_check(cvh_context *const *ctxs, int n, cvh_context *c, int radius, const char *what, const char *who)
{
  if (radius < 1 || radius > CVH_LOC_RADIUS_MAX)
    return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: %sradius = %d, must be 1 .. %d", what, who, radius, CVH_LOC_RADIUS_MAX);
  if (c->state_bits == 32) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: %sthe context has \"state\" = 32: the call iterates an FP64 level set", what, who);
  if (c->n >= ((size_t)1 << 28)) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: %s%d x %d is too large, h * w must stay below 2^28", what, who, c->h, c->w);
  if (!c->have_image) return batch_fail(ctxs, n, CVH_ERR_STATE, "%s: %sthe context has no image (call cvh_set_image first)", what, who);
  if (!c->have_u) return batch_fail(ctxs, n, CVH_ERR_STATE, "%s: %sthe context has no level set", what, who);
  return CVH_OK;
}

size_t partial_bytes(const CvhLocGeom &g) { return align_up((size_t)g.nitems * sizeof(double), 256); }

// the members settled, their FP64 mirrors fresh, their workspaces there
int loc_ready(cvh_context *const *ctxs, int n, const char *what, const CvhLocGeom *g)
{
  HIPCHK(ctxs[0], hipSetDevice(ctxs[0]->device));
  int rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    const size_t bytes = kLocStateBytes + partial_bytes(g[i]) + c->n * ((1 + c->C) * sizeof(unsigned long long) + c->C * sizeof(unsigned));
    const bool fresh = !c->d_localized;
    rc = ensure_workspace(c, &c->d_localized, bytes, "localised-regions", false);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: %s", what, c->err);
    if (fresh) HIPCHK(c, hipMemsetAsync(c->d_localized, 0, kLocStateBytes, c->stream));   // a state block never holds what hipMalloc left there
  }
  return CVH_OK;
}

// everything of a member's record but the state slot, the trace, the prefix block counts and the planes of cvh_localized_means;
// u[0] is the buffer that holds the level set now
void loc_args(const cvh_context *c, int radius, const CvhLocGeom &g, CvhLocArgs *m)
{
  memset(m, 0, sizeof(*m));
  const int cur = current_buffer(c);
  m->u[0] = c->d_u[cur]; m->u[1] = c->d_u[cur ^ 1];
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

// the sections of a class's two grids: record r owns its member's own grids behind those of the records of its class before it
void loc_lay_out(CvhLocArgs *recs, MarchClass *cls)
{
  for (int k = 0; k < kMarchClasses; ++k) {
    unsigned wave = 0, rows = 0;
    for (int r = cls[k].first; r < cls[k].first + cls[k].n; ++r) {
      recs[r].wave_first = wave; wave += recs[r].g.grid;
      recs[r].row_first = rows; rows += recs[r].g.row_grid;
    }
    cls[k].grid = wave; cls[k].grid2 = rows;
  }
}

// one launch per class present: the row pass and the wave kernel of kind `kind` (and, in a run, the finalise) for all its members.
// one: the call's only record on the host, which then travels by value
int loc_launches(cvh_context *lead, const CvhLocArgs *d_recs, const MarchClass *cls, int parity, int kind, const CvhLocArgs *one)
{
  for (int k = 0; k < kMarchClasses; ++k) {
    const MarchClass &q = cls[k];
    if (!q.n) continue;
    const CvhLocArgs *tab = d_recs + q.first;
    const int fast = kind == CVH_LOC_TSUM ? 0 : q.fast;   // (T_k: wq = 1, no form of H_eps; the MEANS wave kernel has none either)
    HIPCHK(lead, cvh_launch_loc_rows(tab, q.n, q.grid2, parity, q.C, fast, kind, lead->stream, one));
    HIPCHK(lead, cvh_launch_loc_wave(tab, q.n, q.grid, parity, q.C, kind == CVH_LOC_STEP ? fast : 0, kind, lead->stream, one));
    if (kind == CVH_LOC_STEP) HIPCHK(lead, cvh_launch_loc_finalize(tab, q.n, lead->stream, one));
  }
  return CVH_OK;
}

// The batch's own refusals, then every member's; ctxs[0 .. n-1] are listed, distinct and on one device afterwards
int loc_batch_check(cvh_context *const *ctxs, int n, const int *radius, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  if (!radius) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: radius is NULL", what);
  unsigned long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    rc = loc_check(ctxs, n, ctxs[i], radius[i], what, member_prefix(i).c_str());
    if (rc != CVH_OK) return rc;
    const CvhLocGeom g = cvh_loc_geometry(ctxs[i]->h, ctxs[i]->w, radius[i]);
    blocks += std::max(g.grid, g.row_grid);
    if (blocks >= (1ull << 31)) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: the members up to this one need 2^31 workgroups or more in one launch", what, i);
  }
  return CVH_OK;
}

// ctxs[0 .. n-1] have passed loc_check (and, for n > 1, loc_batch_check); who(i) opens what a message says about member i
int localized_run(cvh_context *const *ctxs, int n, const int *radius, int max_steps, int *steps_done, double *norms, double *const *traces,
                  int trace_rows, int *rows, const char *what, const std::function<std::string(int)> &who)
{
  cvh_context *lead = ctxs[0];
  MarchRun run{ctxs, n, 1, what, who};
  int rc = run.begin(max_steps, traces, trace_rows, rows);
  if (rc != CVH_OK) return rc;
  std::vector<CvhLocGeom> g((size_t)n);
  for (int i = 0; i < n; ++i) g[i] = cvh_loc_geometry(ctxs[i]->h, ctxs[i]->w, radius[i]);
  rc = loc_ready(ctxs, n, what, g.data());
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {   // the stop norms (taken again where the planes changed on the device)
    rc = prepare_host(ctxs[i]);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: %s%s", what, who(i).c_str(), ctxs[i]->err);
  }
  rc = run.open([&](int i) { return &ctxs[i]->loc_trace; }, [](int) { return 1; }, sizeof(CvhLocArgs), kLocSlotBytes);
  if (rc != CVH_OK) return rc;
  std::vector<int> order;
  MarchClass cls[kMarchClasses];
  march_classes(ctxs, n, 1, &order, cls);
  CvhLocArgs *recs = (CvhLocArgs *)run.record(0);
  for (int r = 0; r < n; ++r) {
    const int i = order[r];
    loc_args(ctxs[i], radius[i], g[i], &recs[r]);
    recs[r].st_mirror = (CvhLocState *)run.d_state(i);
    recs[r].trace = run.d_trace[i]; recs[r].trace_cap = run.trace_cap[i];
    // no launch in front of the first iteration writes the state block (the four-phase flow's initial finalise does): zeroed here
    HIPCHK(lead, hipMemsetAsync(ctxs[i]->d_localized, 0, kLocStateBytes, lead->stream));
  }
  loc_lay_out(recs, cls);
  // ONE member: its record travels by value -- u[0] read, u[1] written, swapped here per iteration -- nothing is uploaded, and the host
  // reads the member's own state block: the single call's launches as they were before the batch existed
  CvhLocArgs *one = n == 1 ? recs : nullptr;
  double *const pair[2] = {recs[0].u[0], recs[0].u[1]};
  if (one) run.own_state = ctxs[0]->d_localized;
  else rc = run.upload();
  if (rc != CVH_OK) return rc;
  const CvhLocArgs *d_recs = (const CvhLocArgs *)run.d_record(0);
  rc = loc_launches(lead, d_recs, cls, 0, CVH_LOC_TSUM, one);   // T_k, once per call: a row pass with wq = 1 and the wave kernel's vertical sums of it
  if (rc != CVH_OK) return rc;
  rc = run.iterate([&](int parity) {
    if (one) { one->u[0] = pair[parity]; one->u[1] = pair[parity ^ 1]; }
    return loc_launches(lead, d_recs, cls, parity, CVH_LOC_STEP, one);
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const CvhLocState *st = (const CvhLocState *)run.state(i);
    if (steps_done) steps_done[i] = st->run.steps_done;
    if (norms) norms[i] = st->norm;
  }
  return CVH_OK;
}

int localized_means(cvh_context *c, int radius, double *c1, double *c2, uint64_t *wq, uint64_t *a, uint64_t *s, const char *what)
{
  cvh_context *ctxs[1] = {c};
  int rc = loc_check(ctxs, 1, c, radius, what, "");
  if (rc != CVH_OK) return rc;
  if (!c1 && !c2 && !wq && !a && !s) return batch_fail(ctxs, 1, CVH_ERR_ARG, "%s: every output is NULL", what);
  const CvhLocGeom g = cvh_loc_geometry(c->h, c->w, radius);
  rc = loc_ready(ctxs, 1, what, &g);
  if (rc != CVH_OK) return rc;
  // one record, by value: the launches of a single run, which never read the state block here
  CvhLocArgs m;
  loc_args(c, radius, g, &m);
  MarchClass cls[kMarchClasses];
  std::vector<int> order;
  march_classes(ctxs, 1, 1, &order, cls);
  loc_lay_out(&m, cls);
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
  auto body = [&]() -> int {
    int r2 = open_call(ctxs, 1, nullptr);
    if (r2 != CVH_OK) return r2;
    r2 = loc_launches(c, nullptr, cls, 0, CVH_LOC_TSUM, &m);
    if (r2 != CVH_OK) return r2;
    r2 = loc_launches(c, nullptr, cls, 0, CVH_LOC_MEANS, &m);
    if (r2 != CVH_OK) return r2;
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
  return guarded_one(ctx, "cvh_localized_run", [&](const char *what) -> int {
    cvh_context *ctxs[1] = {ctx};
    const int rc = loc_check(ctxs, 1, ctx, radius, what, "");
    if (rc != CVH_OK) return rc;
    double *traces[1] = {trace};
    return localized_run(ctxs, 1, &radius, max_steps, steps_done, norm, traces, trace_rows, rows, what, [](int) { return std::string(); });
  });
}

extern "C" int cvh_localized_run_batch(cvh_context *const *ctxs, int n, const int *radius, int max_steps, int *steps_done, double *norms,
                                       double *const *traces, int trace_rows, int *rows)
{
  static const char what[] = "cvh_localized_run_batch";
  return guarded(nullptr, 0, what, [&]() -> int {
    const int rc = loc_batch_check(ctxs, n, radius, what);
    if (rc != CVH_OK) return rc;
    return localized_run(ctxs, n, radius, max_steps, steps_done, norms, traces, trace_rows, rows, what, member_prefix);
  });
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
