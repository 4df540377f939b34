// convex_run.hip — host side of the convex relaxation (include/chanvese_hip.h, "Convex relaxation"; kernels in convex_kernels.hip).
// A call checks its members and their parameters here, and ConvexFlow describes the flow to march_flow.h's one call sequence: per
// iteration and (channel count, math mode) class two launches on the leader's stream over the members of that class -- the step kernel
// and the finalise, one workgroup per member; in front of iteration 0 the start launch (v0, vbar0, q = 0 and the sums of v0; a resumed
// member's workgroups return at once) and a finalise, which writes the whole state block or, for a resumed member, its run counters
// alone; behind the last chunk a bake launch per member, u = v - 0.5 into the buffer a new level set lands in.
// cvh_convex_run is the batch of one member, which the sequence hands to the by-value kernels.
// The workspace, kept by each context: [state block][the items' rows of partial sums][v][vbar, qx, qy of set 0][vbar, qx, qy of set 1];
// the state block is never zeroed here -- a resumed call reads what the last one left.
#include "march_flow.h"

namespace {

struct ConvexFlow {
  using Args = CvhCvxArgs; using State = CvhCvxState; using Geom = CvhMpGeom;   // (the four-phase partition)
  static constexpr size_t kStateBytes = 256;
  static constexpr size_t kSlotBytes = 128;   // a member's slot of the leader's state table
  static constexpr int kPer = 1;
  static constexpr const char *kWorkspace = "convex";
  static constexpr bool kZeroState = false;
  cvh_context *const *all;
  const cvh_convex_params *par;   // [n]

  static void **workspace(cvh_context *c) { return &c->d_convex; }
  static DeviceTable *trace_table(cvh_context *c) { return &c->cvx_trace; }
  static int row_width(int C) { return 2 * C + 1; }
  static unsigned blocks(const Geom &g) { return g.grid; }
  static MarchSections sections(Args &r) { return {{&r.first, nullptr}, {r.g.grid, 0}}; }
  static void norms_out(const State &st, int i, double *norms) { norms[i] = st.norm; }
  static size_t planes_offset(const cvh_context *c, const Geom &g) { return kStateBytes + align_up((size_t)g.nitems * cvh_cvx_nsums(c->C) * sizeof(double), 256); }
  Geom geometry(int i) const { return cvh_mp_geometry(all[i]->h, all[i]->w); }
  size_t workspace_bytes(int i, const Geom &g) const { return planes_offset(all[i], g) + 7 * all[i]->n * sizeof(double); }

  // plane j of c's relaxation state: 0 v, then vbar, qx, qy of set 0 and of set 1
  static double *plane(const cvh_context *c, int j)
  {
    return (double *)((unsigned char *)c->d_convex + planes_offset(c, cvh_mp_geometry(c->h, c->w))) + (size_t)j * c->n;
  }

  // What every call refuses for member i of n before anything is touched; `who` opens what the message says ("" or "member 3: ")
  int rules(int n, int i, const char *what, const char *who) const
  {
    const cvh_context *c = all[i];
    if (!par) return batch_fail(all, n, CVH_ERR_ARG, "%s: the parameters are NULL", what);
    const cvh_convex_params &p = par[i];
    if (!(isfinite(p.tau) && p.tau > 0.0)) return batch_fail(all, n, CVH_ERR_ARG, "%s: %stau must be finite and positive, got %g", what, who, p.tau);
    if (!(isfinite(p.sigma) && p.sigma > 0.0)) return batch_fail(all, n, CVH_ERR_ARG, "%s: %ssigma must be finite and positive, got %g", what, who, p.sigma);
    if (!(8.0 * p.tau * p.sigma <= 1.0))
      return batch_fail(all, n, CVH_ERR_ARG, "%s: %s8 tau sigma must not exceed 1, got tau = %g, sigma = %g", what, who, p.tau, p.sigma);
    if (isnan(p.stop_rms)) return batch_fail(all, n, CVH_ERR_ARG, "%s: %sstop_rms is NaN", what, who);
    if (p.means_every < 0) return batch_fail(all, n, CVH_ERR_ARG, "%s: %smeans_every must not be negative, got %d", what, who, p.means_every);
    if (c->state_bits == 32) return batch_fail(all, n, CVH_ERR_ARG, "%s: %sthe context has \"state\" = 32: the call iterates FP64 planes", what, who);
    if (c->n >= ((size_t)1 << 28)) return batch_fail(all, n, CVH_ERR_ARG, "%s: %s%d x %d is too large, h * w must stay below 2^28", what, who, c->h, c->w);
    if (!c->have_image) return batch_fail(all, n, CVH_ERR_STATE, "%s: %sthe context has no image (call cvh_set_image first)", what, who);
    if (!p.resume && !c->have_u) return batch_fail(all, n, CVH_ERR_STATE, "%s: %sthe context has no level set", what, who);
    if (p.resume && !c->have_convex)
      return batch_fail(all, n, CVH_ERR_STATE, "%s: %sthe context has no relaxation state to resume (run once with resume = 0)", what, who);
    if (p.use_edge && !c->have_gq)
      return batch_fail(all, n, CVH_ERR_STATE, "%s: %sthe context has no edge plane (call cvh_set_edge_map or cvh_edge_map first)", what, who);
    return CVH_OK;
  }

  // the set a call starts from: the one the last call left current, or -- a fresh start -- set 0
  int first_set(int i) const { return par[i].resume ? all[i]->convex_cur : 0; }

  // u[0] is the set that holds vbar and q now (a fresh start writes it)
  void args(int i, const Geom &g, Args *m) const
  {
    const cvh_context *c = all[i];
    const cvh_convex_params &p = par[i];
    memset(m, 0, sizeof(*m));
    const int cur = first_set(i);
    for (int e = 0; e < 2; ++e) {
      const int set = cur ^ e;
      m->u[e] = CvhCvxBufs{plane(c, 1 + 3 * set), plane(c, 2 + 3 * set), plane(c, 3 + 3 * set)};
    }
    m->v = plane(c, 0);
    m->levelset = c->d_u[current_buffer(c)];
    for (int k = 0; k < c->C; ++k) { m->img[k] = c->d_img[k]; m->sum_img[k] = c->sum_img[k]; m->lambda1[k] = c->p.lambda1[k]; m->lambda2[k] = c->p.lambda2[k]; }
    m->gq = p.use_edge ? c->d_gq : nullptr;
    m->st = (CvhCvxState *)c->d_convex;
    m->partials = (double *)((unsigned char *)c->d_convex + kStateBytes);
    m->h = c->h; m->w = c->w;
    m->g = g;
    m->tau = p.tau; m->sigma = p.sigma; m->mu = c->p.mu; m->nu = c->p.nu;
    m->stop = p.stop_rms < 0.0 ? -1.0 : p.stop_rms * sqrt((double)c->n);
    m->npix = (double)c->n;
    m->means_every = p.means_every; m->resume = p.resume ? 1 : 0;
  }

  static int launches(cvh_context *lead, const Args *tab, const MarchClass &q, int parity, bool init, const Args *one)
  {
    if (init) { if (!one || !one->resume) HIPCHK(lead, cvh_launch_cvx_start(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one)); }
    else HIPCHK(lead, cvh_launch_cvx_step(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one));
    HIPCHK(lead, cvh_launch_cvx_finalize(tab, q.n, q.C, init ? 1 : 0, lead->stream, one));
    return CVH_OK;
  }
  static int before(cvh_context *lead, const Args *tab, const MarchClass &q, const Args *one) { return launches(lead, tab, q, 0, true, one); }
  static int step(cvh_context *lead, const Args *tab, const MarchClass &q, int parity, const Args *one) { return launches(lead, tab, q, parity, false, one); }
};
static_assert(sizeof(CvhCvxState) <= ConvexFlow::kStateBytes, "the workspace's first section holds the state block");
static_assert(sizeof(CvhCvxState) <= ConvexFlow::kSlotBytes, "a slot of the state table holds the state block");

// the run of n checked members: behind the last chunk every member's u = v - 0.5 goes into the buffer a new level set lands in (the
// in-place level-set writers' way), and the contexts remember their relaxation state and which set is current
int convex_run(const ConvexFlow &flow, int n, int max_steps, int *steps_done, double *norms, double *const *traces, int trace_rows, int *rows,
               const char *what, const std::function<std::string(int)> &who)
{
  cvh_context *const *all = flow.all;
  std::vector<int> done((size_t)n, 0);
  const int rc = march_run(flow, n, max_steps, done.data(), norms, traces, trace_rows, rows, what, who, [&](int k, int) -> int {
    cvh_context *c = all[k];
    HIPCHK(all[0], cvh_launch_cvx_bake(ConvexFlow::plane(c, 0), c->d_u[c->chain_pb & 1], c->n, all[0]->stream));
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    all[i]->convex_cur = (flow.first_set(i) + done[i]) & 1;
    all[i]->have_convex = true;
    if (steps_done) steps_done[i] = done[i];
  }
  return CVH_OK;
}

}  // namespace

extern "C" int cvh_convex_run(cvh_context *ctx, int max_steps, const cvh_convex_params *params, int *steps_done, double *norm, double *trace,
                              int trace_rows, int *rows)
{
  return guarded_one(ctx, "cvh_convex_run", [&](const char *what) -> int {
    cvh_context *ctxs[1] = {ctx};
    const ConvexFlow flow{ctxs, params};
    const int rc = flow.rules(1, 0, what, "");
    if (rc != CVH_OK) return rc;
    double *traces[1] = {trace};
    return convex_run(flow, 1, max_steps, steps_done, norm, traces, trace_rows, rows, what, [](int) { return std::string(); });
  });
}

extern "C" int cvh_convex_run_batch(cvh_context *const *ctxs, int n, int max_steps, const cvh_convex_params *params, int *steps_done, double *norms,
                                    double *const *traces, int trace_rows, int *rows)
{
  static const char what[] = "cvh_convex_run_batch";
  return guarded(nullptr, 0, what, [&]() -> int {
    int rc = members_check(ctxs, n, what, kMembersListed);   // listed, distinct and on one device afterwards
    if (rc != CVH_OK) return rc;
    const ConvexFlow flow{ctxs, params};
    rc = march_batch_rules(flow, n, what);
    if (rc != CVH_OK) return rc;
    return convex_run(flow, n, max_steps, steps_done, norms, traces, trace_rows, rows, what, member_prefix);
  });
}

extern "C" int cvh_get_relaxed(cvh_context *ctx, double *v, double *qx, double *qy)
{
  return guarded_one(ctx, "cvh_get_relaxed", [&](const char *what) -> int {
    if (!ctx->have_convex) return fail(ctx, CVH_ERR_STATE, "%s: the context has no relaxation state (call cvh_convex_run first)", what);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = settle(ctx);
    if (rc != CVH_OK) return rc;
    double *const out[3] = {v, qx, qy};
    const int from[3] = {0, 2 + 3 * ctx->convex_cur, 3 + 3 * ctx->convex_cur};
    for (int j = 0; j < 3; ++j)
      if (out[j]) HIPCHK(ctx, hipMemcpyAsync(out[j], ConvexFlow::plane(ctx, from[j]), ctx->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return CVH_OK;
  });
}

// ordered behind `stream` and in front of what is enqueued on it later; no host wait
extern "C" int cvh_get_relaxed_device(cvh_context *ctx, double *d_v, void *stream)
{
  return guarded_one(ctx, "cvh_get_relaxed_device", [&](const char *what) -> int {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = element_pointer_check(&ctx, 1, 0, d_v, sizeof(double), what);
    if (rc != CVH_OK) return rc;
    if (!ctx->have_convex) return fail(ctx, CVH_ERR_STATE, "%s: the context has no relaxation state (call cvh_convex_run first)", what);
    rc = open_call(&ctx, 1, stream);
    if (rc != CVH_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_v, ConvexFlow::plane(ctx, 0), ctx->n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return close_call(&ctx, 1, stream, true);
  });
}

extern "C" void cvh_convex_geometry(int h, int w, int *cols, int *strip_rows, int *items) { march_strip_geometry(h, w, cols, strip_rows, items); }
