// localized_run.hip — host side of the localised-regions calls (include/chanvese_hip.h, "Localised regions"; kernels in
// localized_kernels.hip).  A call checks its members here, and LocFlow describes the flow to march_flow.h's one call sequence (ready,
// records, lay-out, iterations, results): per iteration and (channel count, math mode) class three launches on the leader's stream --
// row pass, step, finalise -- over the members of that class, on two grids; in front of iteration 0 the planes T_k, once per call.  No
// launch there writes the state block, so the sequence zeroes it (kZeroState).  cvh_localized_run is the batch of one member, which the
// sequence hands to the by-value kernels; cvh_localized_means takes its record and launches from the same routines.
// The workspace, kept by each context: [state block][the items' partial sums][1 + C planes of 8 bytes: the horizontal window sums][C
// planes of 4 bytes: T_k] -- 8 + 12 C bytes per pixel, whatever the radius.  The table of a call -- the members' argument records and
// their state slots -- is the leader's (MarchRun).
#include "march_flow.h"

namespace {

struct LocFlow {
  using Args = CvhLocArgs; using State = CvhLocState; using Geom = CvhLocGeom;
  static constexpr size_t kStateBytes = 256;
  static constexpr size_t kSlotBytes = 64;   // a member's slot of the leader's state table
  static constexpr int kPer = 1;
  static constexpr const char *kWorkspace = "localised-regions";
  static constexpr bool kZeroState = true;   // a fresh workspace's on the member's stream, every run's on the leader's behind open
  cvh_context *const *all;
  const int *radius;   // per member

  static void **workspace(cvh_context *c) { return &c->d_localized; }
  static DeviceTable *trace_table(cvh_context *c) { return &c->loc_trace; }
  static int row_width(int) { return 1; }
  static unsigned blocks(const Geom &g) { return std::max(g.grid, g.row_grid); }
  static MarchSections sections(Args &r) { return {{&r.wave_first, &r.row_first}, {r.g.grid, r.g.row_grid}}; }
  static void norms_out(const State &st, int i, double *norms) { norms[i] = st.norm; }
  static size_t partial_bytes(const Geom &g) { return align_up((size_t)g.nitems * sizeof(double), 256); }
  Geom geometry(int i) const { return cvh_loc_geometry(all[i]->h, all[i]->w, radius[i]); }
  size_t workspace_bytes(int i, const Geom &g) const
  {
    return kStateBytes + partial_bytes(g) + all[i]->n * ((1 + all[i]->C) * sizeof(unsigned long long) + all[i]->C * sizeof(unsigned));
  }

  // What every call refuses for member i of n before anything is touched; `who` opens what the message says ("" or "member 3: ")
  int rules(int n, int i, const char *what, const char *who) const
  {
    if (radius[i] < 1 || radius[i] > CVH_LOC_RADIUS_MAX)
      return batch_fail(all, n, CVH_ERR_ARG, "%s: %sradius = %d, must be 1 .. %d", what, who, radius[i], CVH_LOC_RADIUS_MAX);
    return march_rules(all, n, all + i, 1, what, who, true);
  }

  // (the planes of cvh_localized_means stay null); u[0] is the buffer that holds the level set now
  void args(int i, const Geom &g, Args *m) const
  {
    const cvh_context *c = all[i];
    memset(m, 0, sizeof(*m));
    const int cur = current_buffer(c);
    m->u[0] = c->d_u[cur]; m->u[1] = c->d_u[cur ^ 1];
    for (int k = 0; k < c->C; ++k) m->img[k] = c->d_img[k];
    unsigned char *ws = (unsigned char *)c->d_localized;
    m->st = (CvhLocState *)ws;
    m->partials = (double *)(ws + kStateBytes);
    m->hw = (unsigned long long *)(ws + kStateBytes + partial_bytes(g));
    m->tsum = (unsigned *)(m->hw + (size_t)(1 + c->C) * c->n);
    m->h = c->h; m->w = c->w; m->radius = radius[i];
    m->g = g;
    march_params(c, &m->alpha, &m->beta, &m->gamma, m->lambda1, m->lambda2, &m->stop);
    fill_front_args(c, &m->f);
  }

  // the row pass and the wave kernel of kind `kind` (and, in a run, the finalise) for a class's members
  static int launches(cvh_context *lead, const Args *tab, const MarchClass &q, int parity, int kind, const Args *one)
  {
    const int fast = kind == CVH_LOC_TSUM ? 0 : q.fast;   // (T_k: wq = 1, no form of H_eps; the MEANS wave kernel has none either)
    HIPCHK(lead, cvh_launch_loc_rows(tab, q.n, q.grid2, parity, q.C, fast, kind, lead->stream, one));
    HIPCHK(lead, cvh_launch_loc_wave(tab, q.n, q.grid, parity, q.C, kind == CVH_LOC_STEP ? fast : 0, kind, lead->stream, one));
    if (kind == CVH_LOC_STEP) HIPCHK(lead, cvh_launch_loc_finalize(tab, q.n, lead->stream, one));
    return CVH_OK;
  }
  // T_k, once per call: a row pass with wq = 1 and the wave kernel's vertical sums of it
  static int before(cvh_context *lead, const Args *tab, const MarchClass &q, const Args *one) { return launches(lead, tab, q, 0, CVH_LOC_TSUM, one); }
  static int step(cvh_context *lead, const Args *tab, const MarchClass &q, int parity, const Args *one) { return launches(lead, tab, q, parity, CVH_LOC_STEP, one); }
};
static_assert(sizeof(CvhLocState) <= LocFlow::kStateBytes, "the workspace's first section holds the state block");
static_assert(sizeof(CvhLocState) <= LocFlow::kSlotBytes, "a slot of the state table holds the state block");

int localized_means(cvh_context *c, int radius, double *c1, double *c2, uint64_t *wq, uint64_t *a, uint64_t *s, const char *what)
{
  cvh_context *ctxs[1] = {c};
  const LocFlow flow{ctxs, &radius};
  int rc = flow.rules(1, 0, what, "");
  if (rc != CVH_OK) return rc;
  if (!c1 && !c2 && !wq && !a && !s) return batch_fail(ctxs, 1, CVH_ERR_ARG, "%s: every output is NULL", what);
  // one record, by value: the launches of a single run, which never read the state block here
  CvhLocArgs m;
  MarchClass cls[kMarchClasses];
  rc = march_single(flow, what, &m, cls);
  if (rc != CVH_OK) return rc;
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
    auto pass = [&](int kind) {
      return march_each_class((const CvhLocArgs *)nullptr, cls, [&](const CvhLocArgs *tab, const MarchClass &q) { return LocFlow::launches(c, tab, q, 0, kind, &m); });
    };
    int r2 = open_call(ctxs, 1, nullptr);
    if (r2 != CVH_OK) return r2;
    r2 = pass(CVH_LOC_TSUM);
    if (r2 != CVH_OK) return r2;
    r2 = pass(CVH_LOC_MEANS);
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
    const LocFlow flow{ctxs, &radius};
    const int rc = flow.rules(1, 0, what, "");
    if (rc != CVH_OK) return rc;
    double *traces[1] = {trace};
    return march_run(flow, 1, max_steps, steps_done, norm, traces, trace_rows, rows, what, [](int) { return std::string(); });
  });
}

extern "C" int cvh_localized_run_batch(cvh_context *const *ctxs, int n, const int *radius, int max_steps, int *steps_done, double *norms,
                                       double *const *traces, int trace_rows, int *rows)
{
  static const char what[] = "cvh_localized_run_batch";
  return guarded(nullptr, 0, what, [&]() -> int {
    int rc = members_check(ctxs, n, what, kMembersListed);   // listed, distinct and on one device afterwards
    if (rc != CVH_OK) return rc;
    if (!radius) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: radius is NULL", what);
    const LocFlow flow{ctxs, radius};
    rc = march_batch_rules(flow, n, what);
    if (rc != CVH_OK) return rc;
    return march_run(flow, n, max_steps, steps_done, norms, traces, trace_rows, rows, what, member_prefix);
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
