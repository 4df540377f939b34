// multiphase_run.hip — host side of the four-phase calls (include/chanvese_hip.h, "Four phases"): two contexts A and B hold phi1 and
// phi2 of a Vese-Chan pair and are iterated together by multiphase_kernels.hip.  The pair has no object of its own: a call checks its
// pairs here, and MpFlow describes the flow to march_flow.h's one call sequence (ready, records, lay-out, iterations, results).  Per
// iteration and (channel count, math mode) class two launches on A0's stream over the pairs of that class: the step kernel (the update
// of both level sets and the items' partial sums of the new pair) and the finalise, one workgroup per pair (means, norms, trace row,
// count, stop flag into the state block of A's workspace and its mirror in the leader's state table); in front of iteration 0 the sums
// of the current pairs and a finalise, which writes the whole state block.  cvh_multiphase_run is the batch of one pair, which the
// sequence hands to the by-value kernels; cvh_multiphase_means takes its record and launches from the same routines.
#include "march_flow.h"

namespace {

struct MpFlow {
  using Args = CvhMpArgs; using State = CvhMpState; using Geom = CvhMpGeom;
  static constexpr size_t kStateBytes = 256;   // the workspace: [CvhMpState][the items' rows of partial sums]
  static constexpr size_t kSlotBytes = 128;    // a pair's slot of the leader's state table
  static constexpr int kPer = 2;
  static constexpr const char *kWorkspace = "multiphase";
  static constexpr bool kZeroState = false;
  cvh_context *const *all;   // [A0, B0, A1, B1, ...]

  static void **workspace(cvh_context *a) { return &a->d_multiphase; }
  static DeviceTable *trace_table(cvh_context *a) { return &a->mp_trace; }
  static int row_width(int C) { return 4 * C + 2; }
  static unsigned blocks(const Geom &g) { return g.grid; }
  static MarchSections sections(Args &r) { return {{&r.first, nullptr}, {r.g.grid, 0}}; }
  static void norms_out(const State &st, int i, double *norms) { norms[2 * i] = st.norm[0]; norms[2 * i + 1] = st.norm[1]; }
  Geom geometry(int i) const { return cvh_mp_geometry(all[2 * i]->h, all[2 * i]->w); }
  size_t workspace_bytes(int i, const Geom &g) const { return kStateBytes + (size_t)g.nitems * cvh_mp_nsums(all[2 * i]->C) * sizeof(double); }

  // What every call refuses for pair i of n before anything is touched; the message goes to all[0] and opens with `who`
  int rules(int n, int i, const char *what, const char *who, bool need_images = true) const
  {
    cvh_context *a = all[2 * i], *b = all[2 * i + 1];
    if (a->device != all[0]->device)
      return batch_fail(all, 2 * n, CVH_ERR_ARG, "%s: member %d is on device %d, member 0 on device %d", what, i, a->device, all[0]->device);
    if (a->device != b->device) return batch_fail(all, 2 * n, CVH_ERR_ARG, "%s: %sa is on device %d, b on device %d", what, who, a->device, b->device);
    if (a->h != b->h || a->w != b->w) return batch_fail(all, 2 * n, CVH_ERR_ARG, "%s: %sa is %d x %d, b %d x %d", what, who, a->h, a->w, b->h, b->w);
    if (a->C != b->C) return batch_fail(all, 2 * n, CVH_ERR_ARG, "%s: %sa has %d channel(s), b %d", what, who, a->C, b->C);
    if (a->p.eps != b->p.eps) return batch_fail(all, 2 * n, CVH_ERR_ARG, "%s: %seps must be equal in both contexts, got %g and %g", what, who, a->p.eps, b->p.eps);
    return march_rules(all, 2 * n, all + 2 * i, 2, what, who, need_images);
  }

  // u[0][e] is the buffer that holds the level set now
  void args(int i, const Geom &g, Args *m) const
  {
    const cvh_context *a = all[2 * i];
    memset(m, 0, sizeof(*m));
    for (int k = 0; k < a->C; ++k) m->img[k] = a->d_img[k];
    m->st = (CvhMpState *)a->d_multiphase;
    m->partials = (double *)((unsigned char *)a->d_multiphase + kStateBytes);
    m->h = a->h; m->w = a->w;
    m->g = g;
    for (int e = 0; e < 2; ++e) {
      const cvh_context *c = all[2 * i + e];
      const int cur = current_buffer(c);
      m->u[0][e] = c->d_u[cur]; m->u[1][e] = c->d_u[cur ^ 1];
      march_params(c, &m->alpha[e], &m->beta[e], &m->gamma[e], m->lambda1[e], m->lambda2[e], &m->stop[e]);
    }
    fill_front_args(a, &m->f);
  }

  // init: the sums of the current pairs (parity 0) and the means they give into the state blocks; else one iteration of parity `parity`
  static int launches(cvh_context *lead, const Args *tab, const MarchClass &q, int parity, bool init, const Args *one)
  {
    if (init) HIPCHK(lead, cvh_launch_mp_sums(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one));
    else HIPCHK(lead, cvh_launch_mp_step(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one));
    HIPCHK(lead, cvh_launch_mp_finalize(tab, q.n, q.C, init ? 1 : 0, lead->stream, one));
    return CVH_OK;
  }
  static int before(cvh_context *lead, const Args *tab, const MarchClass &q, const Args *one) { return launches(lead, tab, q, 0, true, one); }
  static int step(cvh_context *lead, const Args *tab, const MarchClass &q, int parity, const Args *one) { return launches(lead, tab, q, parity, false, one); }
};
static_assert(sizeof(CvhMpState) <= MpFlow::kStateBytes, "the workspace's first section holds the pair's state block");
static_assert(sizeof(CvhMpState) <= MpFlow::kSlotBytes, "a slot of the state table holds the state block");
static_assert(sizeof(CvhMpState) <= 4 * sizeof(CvhState), "cvh_multiphase_means: the state block comes down into the context's pinned state slots (state_down)");

// a single pair: ctxs[2] = {a, b} is filled here
int pair_check(cvh_context *a, cvh_context *b, const char *what, bool need_images, cvh_context **ctxs)
{
  ctxs[0] = a; ctxs[1] = b;
  if (!a || !b) return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: context %s is NULL", what, a ? "b" : "a");
  if (a == b) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: a and b are the same context (a pair is two contexts)", what);
  return MpFlow{ctxs}.rules(1, 0, what, "", need_images);
}

// The batch's own refusals, then every pair's; *all = [A0, B0, A1, B1, ...], the call's member list, is filled here
int pairs_batch_check(cvh_context *const *as, cvh_context *const *bs, int n, const char *what, std::vector<cvh_context *> *all)
{
  if (!as || !bs || n < 1)
    return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: empty pair list (as = %p, bs = %p, n = %d)", what, (const void *)as, (const void *)bs, n);
  for (int i = 0; i < n; ++i)
    if (!as[i] || !bs[i]) return batch_fail(i ? as : nullptr, i ? 1 : 0, CVH_ERR_ARG, "%s: member %d: context %s is NULL", what, i, as[i] ? "b" : "a");
  all->clear();
  for (int i = 0; i < n; ++i) { all->push_back(as[i]); all->push_back(bs[i]); }
  for (int k = 0; k < 2 * n; ++k)
    for (int j = 0; j < k; ++j)
      if ((*all)[j] == (*all)[k])
        return batch_fail(all->data(), 2 * n, CVH_ERR_ARG, "%s: member %d: context %c is also member %d's context %c (every context may appear once)", what, k / 2,
                          "ab"[k & 1], j / 2, "ab"[j & 1]);
  return march_batch_rules(MpFlow{all->data()}, n, what);
}

int multiphase_means(cvh_context *a, cvh_context *b, double *c, const char *what)
{
  cvh_context *ctxs[2];
  int rc = pair_check(a, b, what, true, ctxs);
  if (rc != CVH_OK) return rc;
  if (!c) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: c is NULL", what);
  CvhMpArgs m;   // one record, by value
  MarchClass cls[kMarchClasses];
  rc = march_single(MpFlow{ctxs}, what, &m, cls);
  if (rc != CVH_OK) return rc;
  rc = open_call(ctxs, 2, nullptr);
  if (rc != CVH_OK) return rc;
  rc = march_each_class((const CvhMpArgs *)nullptr, cls, [&](const CvhMpArgs *tab, const MarchClass &q) { return MpFlow::before(a, tab, q, &m); });
  if (rc != CVH_OK) return rc;
  rc = close_call(ctxs, 2, nullptr, false);
  if (rc != CVH_OK) return rc;
  CvhMpState st;
  rc = state_down(a, a->d_multiphase, &st, sizeof(st));
  if (rc != CVH_OK) return rc;
  for (int ab = 0; ab < 4; ++ab)
    for (int k = 0; k < a->C; ++k) c[ab * a->C + k] = st.c[ab][k];
  return CVH_OK;
}

// one member-table launch on A's stream, ordered behind `stream` and in front of what is enqueued on it later; no host wait
int labels_out(cvh_context *a, cvh_context *b, uint8_t *d_labels, void *stream, const char *what)
{
  cvh_context *ctxs[2];
  int rc = pair_check(a, b, what, false, ctxs);
  if (rc != CVH_OK) return rc;
  HIPCHK(a, hipSetDevice(a->device));
  rc = pointer_check(ctxs, 2, 0, d_labels, what);
  if (rc != CVH_OK) return rc;
  rc = settle_all(ctxs, 2, what);
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(ctxs, 2, what);
  if (rc != CVH_OK) return rc;
  MemberCall call;
  rc = call.begin(ctxs, 2, what);
  if (rc != CVH_OK) return rc;
  call.tab[0].src = a->d_u[current_buffer(a)];
  call.tab[0].src2 = b->d_u[current_buffer(b)];
  call.tab[0].dst = d_labels;
  call.tab[0].nblk = cvh_io_blocks(a->n);   // (b's entry owns no workgroups: the kernel's table is the first entry)
  return call.run(stream, true, false, [&]() -> int { HIPCHK(a, cvh_launch_mp_labels(call.dtab(), 1, call.grid, a->stream)); return CVH_OK; });
}

}  // namespace

extern "C" int cvh_multiphase_run(cvh_context *a, cvh_context *b, int max_steps, int *steps_done, double *norms, double *trace, int trace_rows,
                                  int *rows)
{
  static const char what[] = "cvh_multiphase_run";
  return guarded(nullptr, 0, what, [&]() -> int {
    cvh_context *ctxs[2];
    const int rc = pair_check(a, b, what, true, ctxs);
    if (rc != CVH_OK) return rc;
    double *traces[1] = {trace};
    return march_run(MpFlow{ctxs}, 1, max_steps, steps_done, norms, traces, trace_rows, rows, what,
                     [](int k) { return std::string(k ? "context b: " : "context a: "); });
  });
}

extern "C" int cvh_multiphase_run_batch(cvh_context *const *as, cvh_context *const *bs, int n, int max_steps, int *steps_done, double *norms,
                                        double *const *traces, int trace_rows, int *rows)
{
  static const char what[] = "cvh_multiphase_run_batch";
  return guarded(nullptr, 0, what, [&]() -> int {
    std::vector<cvh_context *> all;
    const int rc = pairs_batch_check(as, bs, n, what, &all);
    if (rc != CVH_OK) return rc;
    return march_run(MpFlow{all.data()}, n, max_steps, steps_done, norms, traces, trace_rows, rows, what,
                     [](int k) { return member_prefix(k / 2) + (k & 1 ? "context b: " : "context a: "); });
  });
}

extern "C" int cvh_multiphase_means(cvh_context *a, cvh_context *b, double *c)
{
  static const char what[] = "cvh_multiphase_means";
  return guarded(nullptr, 0, what, [&]() { return multiphase_means(a, b, c, what); });
}

extern "C" int cvh_multiphase_labels_device(cvh_context *a, cvh_context *b, uint8_t *d_labels, void *stream)
{
  static const char what[] = "cvh_multiphase_labels_device";
  return guarded(nullptr, 0, what, [&]() { return labels_out(a, b, d_labels, stream, what); });
}

extern "C" int cvh_multiphase_labels(cvh_context *a, cvh_context *b, uint8_t *labels)
{
  static const char what[] = "cvh_multiphase_labels";
  return guarded(nullptr, 0, what, [&]() -> int {
    cvh_context *ctxs[2];
    const int rc = pair_check(a, b, what, false, ctxs);   // (first: a's buffer is touched below)
    if (rc != CVH_OK) return rc;
    if (!labels) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: labels is NULL", what);
    return mask_to_host(a, labels, [&]() { return labels_out(a, b, a->d_mask, a->stream, what); });
  });
}

extern "C" void cvh_multiphase_geometry(int h, int w, int *cols, int *strip_rows, int *items) { march_strip_geometry(h, w, cols, strip_rows, items); }
