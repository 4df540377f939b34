// geodesic_run.hip — host side of the edge-weighted iteration (include/chanvese_hip.h, "Edge-weighted length"; kernels in
// geodesic_kernels.hip).  A call checks everything, settles its members as the getters do and takes their initial sums itself;
// cvh_geodesic_run_batch then hands the iterations to march_run.hip's driver: per iteration and (channel count, math mode) class two
// launches on the leader's stream over the members of that class -- the step kernel (the update and the items' partial sums of the new
// level set) and the finalise, one workgroup per member.  cvh_geodesic_run is the batch of one member: one host path.  A call with ONE
// member hands its record to the by-value kernels: no upload, no mirror, the host reads the member's own state block.
// The workspace, kept by each context: [state block][the items' rows of partial sums].
#include "cvh_host.h"

namespace {

constexpr size_t kGeoStateBytes = 256;
constexpr size_t kGeoSlotBytes = 64;    // a member's slot of the leader's state table
static_assert(sizeof(CvhGeoState) <= kGeoStateBytes, "the workspace's first section holds the state block");
static_assert(sizeof(CvhGeoState) <= kGeoSlotBytes, "a slot of the state table holds the state block");

// What every call refuses for a member before anything is touched; `who` opens what the message says ("" or "member 3: ")
int geo_check(cvh_context *const *ctxs, int n, cvh_context *c, const char *what, const char *who)
{
  if (c->state_bits == 32) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: %sthe context has \"state\" = 32: the call iterates an FP64 level set", what, who);
  if (c->n >= ((size_t)1 << 28)) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: %s%d x %d is too large, h * w must stay below 2^28", what, who, c->h, c->w);
  if (!c->have_image) return batch_fail(ctxs, n, CVH_ERR_STATE, "%s: %sthe context has no image (call cvh_set_image first)", what, who);
  if (!c->have_u) return batch_fail(ctxs, n, CVH_ERR_STATE, "%s: %sthe context has no level set", what, who);
  if (!c->have_gq) return batch_fail(ctxs, n, CVH_ERR_STATE, "%s: %sthe context has no edge plane (call cvh_set_edge_map or cvh_edge_map first)", what, who);
  return CVH_OK;
}

// The batch's own refusals, then every member's; ctxs[0 .. n-1] are listed, distinct and on one device afterwards
int geo_batch_check(cvh_context *const *ctxs, int n, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  unsigned long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    rc = geo_check(ctxs, n, ctxs[i], what, member_prefix(i).c_str());
    if (rc != CVH_OK) return rc;
    blocks += cvh_mp_geometry(ctxs[i]->h, ctxs[i]->w).grid;
    if (blocks >= (1ull << 31)) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: the members up to this one need 2^31 workgroups or more in one launch", what, i);
  }
  return CVH_OK;
}

// the members settled, their FP64 mirrors fresh, their workspaces there
int geo_ready(cvh_context *const *ctxs, int n, const char *what, const CvhMpGeom *g)
{
  HIPCHK(ctxs[0], hipSetDevice(ctxs[0]->device));
  int rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    const size_t bytes = kGeoStateBytes + (size_t)g[i].nitems * cvh_geo_nsums(c->C) * sizeof(double);
    rc = ensure_workspace(c, &c->d_geodesic, bytes, "geodesic", false);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: %s", what, c->err);
  }
  return CVH_OK;
}

// everything of a member's record but the state slot, the trace and the prefix block count; u[0] is the buffer that holds the level set now
void geo_args(const cvh_context *c, const CvhMpGeom &g, CvhGeoArgs *m)
{
  memset(m, 0, sizeof(*m));
  const int cur = current_buffer(c);
  m->u[0] = c->d_u[cur]; m->u[1] = c->d_u[cur ^ 1];
  for (int k = 0; k < c->C; ++k) m->img[k] = c->d_img[k];
  m->gq = c->d_gq;
  m->st = (CvhGeoState *)c->d_geodesic;
  m->partials = (double *)((unsigned char *)c->d_geodesic + kGeoStateBytes);
  m->h = c->h; m->w = c->w;
  m->g = g;
  m->alpha = c->p.mu * c->p.dt;          // the folded combine, as fill_args (csv_run.hip)
  m->beta = (1.0 / c->C) * c->p.dt;
  m->gamma = -c->p.nu * c->p.dt;
  for (int k = 0; k < c->C; ++k) { m->lambda1[k] = c->p.lambda1[k]; m->lambda2[k] = c->p.lambda2[k]; m->sum_img[k] = c->sum_img[k]; }
  m->npix = (double)c->n;
  m->stop = c->p.tol * c->stop_norm;
  fill_front_args(c, &m->f);
}

void geo_lay_out(CvhGeoArgs *recs, MarchClass *cls)
{
  for (int k = 0; k < kMarchClasses; ++k) {
    unsigned first = 0;
    for (int r = cls[k].first; r < cls[k].first + cls[k].n; ++r) { recs[r].first = first; first += recs[r].g.grid; }
    cls[k].grid = first;
  }
}

// one launch per kernel and class present, on the leader's stream.  init: the sums of the current level sets (parity 0) and the means
// they give into the state blocks; else one iteration of parity `parity`.  one: the call's only record on the host, which travels by value
int geo_launches(cvh_context *lead, const CvhGeoArgs *d_recs, const MarchClass *cls, int parity, bool init, const CvhGeoArgs *one)
{
  for (int k = 0; k < kMarchClasses; ++k) {
    const MarchClass &q = cls[k];
    if (!q.n) continue;
    const CvhGeoArgs *tab = d_recs + q.first;
    if (init) HIPCHK(lead, cvh_launch_geo_sums(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one));
    else HIPCHK(lead, cvh_launch_geo_step(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one));
    HIPCHK(lead, cvh_launch_geo_finalize(tab, q.n, q.C, init ? 1 : 0, lead->stream, one));
  }
  return CVH_OK;
}

// ctxs[0 .. n-1] have passed geo_check (and, for a batch, geo_batch_check); who(i) opens what a message says about member i
int geodesic_run(cvh_context *const *ctxs, int n, int max_steps, int *steps_done, double *norms, double *const *traces, int trace_rows, int *rows,
                 const char *what, const std::function<std::string(int)> &who)
{
  cvh_context *lead = ctxs[0];
  MarchRun run{ctxs, n, 1, what, who};
  int rc = run.begin(max_steps, traces, trace_rows, rows);
  if (rc != CVH_OK) return rc;
  std::vector<CvhMpGeom> g((size_t)n);
  for (int i = 0; i < n; ++i) g[i] = cvh_mp_geometry(ctxs[i]->h, ctxs[i]->w);
  rc = geo_ready(ctxs, n, what, g.data());
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {   // the stop norms and the plane sums (taken again where the planes changed on the device)
    rc = prepare_host(ctxs[i]);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: %s%s", what, who(i).c_str(), ctxs[i]->err);
  }
  rc = run.open([&](int i) { return &ctxs[i]->geo_trace; }, [&](int i) { return 2 * ctxs[i]->C + 1; }, sizeof(CvhGeoArgs), kGeoSlotBytes);
  if (rc != CVH_OK) return rc;
  std::vector<int> order;
  MarchClass cls[kMarchClasses];
  march_classes(ctxs, n, 1, &order, cls);
  CvhGeoArgs *recs = (CvhGeoArgs *)run.record(0);
  for (int r = 0; r < n; ++r) {
    const int i = order[r];
    geo_args(ctxs[i], g[i], &recs[r]);
    recs[r].st_mirror = (CvhGeoState *)run.d_state(i);
    recs[r].trace = run.d_trace[i]; recs[r].trace_cap = run.trace_cap[i];
  }
  geo_lay_out(recs, cls);
  CvhGeoArgs *one = n == 1 ? recs : nullptr;
  double *const pair[2] = {recs[0].u[0], recs[0].u[1]};
  if (one) run.own_state = ctxs[0]->d_geodesic;
  else rc = run.upload();
  if (rc != CVH_OK) return rc;
  const CvhGeoArgs *d_recs = (const CvhGeoArgs *)run.d_record(0);
  rc = geo_launches(lead, d_recs, cls, 0, true, one);   // (its finalise writes the whole state block)
  if (rc != CVH_OK) return rc;
  rc = run.iterate([&](int parity) {
    if (one) { one->u[0] = pair[parity]; one->u[1] = pair[parity ^ 1]; }
    return geo_launches(lead, d_recs, cls, parity, false, one);
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const CvhGeoState *st = (const CvhGeoState *)run.state(i);
    if (steps_done) steps_done[i] = st->run.steps_done;
    if (norms) norms[i] = st->norm;
  }
  return CVH_OK;
}

}  // namespace

extern "C" int cvh_geodesic_run(cvh_context *ctx, int max_steps, int *steps_done, double *norm, double *trace, int trace_rows, int *rows)
{
  return guarded_one(ctx, "cvh_geodesic_run", [&](const char *what) -> int {
    cvh_context *ctxs[1] = {ctx};
    const int rc = geo_check(ctxs, 1, ctx, what, "");
    if (rc != CVH_OK) return rc;
    double *traces[1] = {trace};
    return geodesic_run(ctxs, 1, max_steps, steps_done, norm, traces, trace_rows, rows, what, [](int) { return std::string(); });
  });
}

extern "C" int cvh_geodesic_run_batch(cvh_context *const *ctxs, int n, int max_steps, int *steps_done, double *norms, double *const *traces,
                                      int trace_rows, int *rows)
{
  static const char what[] = "cvh_geodesic_run_batch";
  return guarded(nullptr, 0, what, [&]() -> int {
    const int rc = geo_batch_check(ctxs, n, what);
    if (rc != CVH_OK) return rc;
    return geodesic_run(ctxs, n, max_steps, steps_done, norms, traces, trace_rows, rows, what, member_prefix);
  });
}

extern "C" void cvh_geodesic_geometry(int h, int w, int *cols, int *strip_rows, int *items)
{
  CvhMpGeom g{0, 0, 0, 0, 0};
  if (h > 0 && w > 0 && (long long)h * w < (1ll << 28)) g = cvh_mp_geometry(h, w);
  if (cols) *cols = CVH_MARCH_COLS;
  if (strip_rows) *strip_rows = g.strip_rows;
  if (items) *items = g.nitems;
}
