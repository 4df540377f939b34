// geodesic_run.hip — host side of the edge-weighted iteration (include/chanvese_hip.h, "Edge-weighted length"; kernels in
// geodesic_kernels.hip).  A call checks its members here, and GeoFlow describes the flow to march_flow.h's one call sequence (ready,
// records, lay-out, iterations, results): per iteration and (channel count, math mode) class two launches on the leader's stream over
// the members of that class -- the step kernel (the update and the items' partial sums of the new level set) and the finalise, one
// workgroup per member; in front of iteration 0 the sums of the current level sets and a finalise, which writes the whole state block.
// cvh_geodesic_run is the batch of one member, which the sequence hands to the by-value kernels.
// The workspace, kept by each context: [state block][the items' rows of partial sums].
#include "march_flow.h"

namespace {

struct GeoFlow {
  using Args = CvhGeoArgs; using State = CvhGeoState; using Geom = CvhMpGeom;   // (the four-phase partition)
  static constexpr size_t kStateBytes = 256;
  static constexpr size_t kSlotBytes = 64;    // a member's slot of the leader's state table
  static constexpr int kPer = 1;
  static constexpr const char *kWorkspace = "geodesic";
  static constexpr bool kZeroState = false;
  cvh_context *const *all;

  static void **workspace(cvh_context *c) { return &c->d_geodesic; }
  static DeviceTable *trace_table(cvh_context *c) { return &c->geo_trace; }
  static int row_width(int C) { return 2 * C + 1; }
  static unsigned blocks(const Geom &g) { return g.grid; }
  static MarchSections sections(Args &r) { return {{&r.first, nullptr}, {r.g.grid, 0}}; }
  static void norms_out(const State &st, int i, double *norms) { norms[i] = st.norm; }
  Geom geometry(int i) const { return cvh_mp_geometry(all[i]->h, all[i]->w); }
  size_t workspace_bytes(int i, const Geom &g) const { return kStateBytes + (size_t)g.nitems * cvh_geo_nsums(all[i]->C) * sizeof(double); }

  // What every call refuses for member i of n before anything is touched; `who` opens what the message says ("" or "member 3: ")
  int rules(int n, int i, const char *what, const char *who) const
  {
    const int rc = march_rules(all, n, all + i, 1, what, who, true);
    if (rc != CVH_OK) return rc;
    if (!all[i]->have_gq) return batch_fail(all, n, CVH_ERR_STATE, "%s: %sthe context has no edge plane (call cvh_set_edge_map or cvh_edge_map first)", what, who);
    return CVH_OK;
  }

  // u[0] is the buffer that holds the level set now
  void args(int i, const Geom &g, Args *m) const
  {
    const cvh_context *c = all[i];
    memset(m, 0, sizeof(*m));
    const int cur = current_buffer(c);
    m->u[0] = c->d_u[cur]; m->u[1] = c->d_u[cur ^ 1];
    for (int k = 0; k < c->C; ++k) { m->img[k] = c->d_img[k]; m->sum_img[k] = c->sum_img[k]; }
    m->gq = c->d_gq;
    m->st = (CvhGeoState *)c->d_geodesic;
    m->partials = (double *)((unsigned char *)c->d_geodesic + kStateBytes);
    m->h = c->h; m->w = c->w;
    m->g = g;
    march_params(c, &m->alpha, &m->beta, &m->gamma, m->lambda1, m->lambda2, &m->stop);
    m->npix = (double)c->n;
    fill_front_args(c, &m->f);
  }

  // init: the sums of the current level sets (parity 0) and the means they give into the state blocks; else one iteration of parity `parity`
  static int launches(cvh_context *lead, const Args *tab, const MarchClass &q, int parity, bool init, const Args *one)
  {
    if (init) HIPCHK(lead, cvh_launch_geo_sums(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one));
    else HIPCHK(lead, cvh_launch_geo_step(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one));
    HIPCHK(lead, cvh_launch_geo_finalize(tab, q.n, q.C, init ? 1 : 0, lead->stream, one));
    return CVH_OK;
  }
  static int before(cvh_context *lead, const Args *tab, const MarchClass &q, const Args *one) { return launches(lead, tab, q, 0, true, one); }
  static int step(cvh_context *lead, const Args *tab, const MarchClass &q, int parity, const Args *one) { return launches(lead, tab, q, parity, false, one); }
};
static_assert(sizeof(CvhGeoState) <= GeoFlow::kStateBytes, "the workspace's first section holds the state block");
static_assert(sizeof(CvhGeoState) <= GeoFlow::kSlotBytes, "a slot of the state table holds the state block");

}  // namespace

extern "C" int cvh_geodesic_run(cvh_context *ctx, int max_steps, int *steps_done, double *norm, double *trace, int trace_rows, int *rows)
{
  return guarded_one(ctx, "cvh_geodesic_run", [&](const char *what) -> int {
    cvh_context *ctxs[1] = {ctx};
    const GeoFlow flow{ctxs};
    const int rc = flow.rules(1, 0, what, "");
    if (rc != CVH_OK) return rc;
    double *traces[1] = {trace};
    return march_run(flow, 1, max_steps, steps_done, norm, traces, trace_rows, rows, what, [](int) { return std::string(); });
  });
}

extern "C" int cvh_geodesic_run_batch(cvh_context *const *ctxs, int n, int max_steps, int *steps_done, double *norms, double *const *traces,
                                      int trace_rows, int *rows)
{
  static const char what[] = "cvh_geodesic_run_batch";
  return guarded(nullptr, 0, what, [&]() -> int {
    int rc = members_check(ctxs, n, what, kMembersListed);   // listed, distinct and on one device afterwards
    if (rc != CVH_OK) return rc;
    const GeoFlow flow{ctxs};
    rc = march_batch_rules(flow, n, what);
    if (rc != CVH_OK) return rc;
    return march_run(flow, n, max_steps, steps_done, norms, traces, trace_rows, rows, what, member_prefix);
  });
}

extern "C" void cvh_geodesic_geometry(int h, int w, int *cols, int *strip_rows, int *items) { march_strip_geometry(h, w, cols, strip_rows, items); }
