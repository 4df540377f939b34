// multiphase_run.hip — host side of the four-phase calls (include/chanvese_hip.h, "Four phases"): two contexts A and B hold phi1 and
// phi2 of a Vese-Chan pair and are iterated together by multiphase_kernels.hip.  The pair has no object of its own: a call checks its
// pairs, settles their contexts as the getters do and takes the pairs' initial sums itself; cvh_multiphase_run_batch then hands the
// iterations to march_run.hip's driver.  Per iteration and (channel count, math mode) class two launches on A0's stream over the pairs
// of that class: the step kernel (the update of both level sets and the items' partial sums of the new pair) and the finalise, one
// workgroup per pair (means, norms, trace row, count, stop flag into the state block of A's workspace and its mirror in the leader's
// state table).  cvh_multiphase_run is the batch of one pair and cvh_multiphase_means takes the same launches: one host path.  A call
// with ONE pair keeps the single call's launches as they were before the batch existed: the record by value (the kernel bodies' second
// entry point), no upload, no mirror, the host reads the pair's own state block (DESIGN.md 4.17b says what the table form cost a plane).
#include "cvh_host.h"

namespace {

constexpr size_t kMpStateBytes = 256;   // the workspace: [CvhMpState][the items' rows of partial sums]
constexpr size_t kMpSlotBytes = 128;    // a pair's slot of the leader's state table
static_assert(sizeof(CvhMpState) <= kMpStateBytes, "the workspace's first section holds the pair's state block");
static_assert(sizeof(CvhMpState) <= kMpSlotBytes, "a slot of the state table holds the state block");
static_assert(sizeof(CvhMpState) <= 4 * sizeof(CvhState), "cvh_multiphase_means: the state block comes down into the context's pinned state slots (state_down)");

// What every call refuses for a pair before anything is touched; the message goes to lead[0] (the call's first context) and opens with
// `who` ("" or "member 3: ")
int pair_rules(cvh_context *const *lead, int nlead, cvh_context *a, cvh_context *b, const char *what, const char *who, bool need_images)
{
  cvh_context *const ab[2] = {a, b};
  if (a->device != b->device) return batch_fail(lead, nlead, CVH_ERR_ARG, "%s: %sa is on device %d, b on device %d", what, who, a->device, b->device);
  if (a->h != b->h || a->w != b->w) return batch_fail(lead, nlead, CVH_ERR_ARG, "%s: %sa is %d x %d, b %d x %d", what, who, a->h, a->w, b->h, b->w);
  if (a->C != b->C) return batch_fail(lead, nlead, CVH_ERR_ARG, "%s: %sa has %d channel(s), b %d", what, who, a->C, b->C);
  if (a->p.eps != b->p.eps) return batch_fail(lead, nlead, CVH_ERR_ARG, "%s: %seps must be equal in both contexts, got %g and %g", what, who, a->p.eps, b->p.eps);
  for (int i = 0; i < 2; ++i)
    if (ab[i]->state_bits == 32) return batch_fail(lead, nlead, CVH_ERR_ARG, "%s: %scontext %c has \"state\" = 32: the pair iterates FP64 level sets", what, who, "ab"[i]);
  if (a->n >= ((size_t)1 << 28)) return batch_fail(lead, nlead, CVH_ERR_ARG, "%s: %s%d x %d is too large, h * w must stay below 2^28", what, who, a->h, a->w);
  for (int i = 0; i < 2; ++i) {
    if (need_images && !ab[i]->have_image)
      return batch_fail(lead, nlead, CVH_ERR_STATE, "%s: %scontext %c has no image (call cvh_set_image first)", what, who, "ab"[i]);
    if (!ab[i]->have_u) return batch_fail(lead, nlead, CVH_ERR_STATE, "%s: %scontext %c has no level set", what, who, "ab"[i]);
  }
  return CVH_OK;
}

// a single pair: ctxs[2] = {a, b} is filled here
int pair_check(cvh_context *a, cvh_context *b, const char *what, bool need_images, cvh_context **ctxs)
{
  ctxs[0] = a; ctxs[1] = b;
  if (!a || !b) return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: context %s is NULL", what, a ? "b" : "a");
  if (a == b) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: a and b are the same context (a pair is two contexts)", what);
  return pair_rules(ctxs, 2, a, b, what, "", need_images);
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
  cvh_context *const *lead = all->data();
  for (int k = 0; k < 2 * n; ++k)
    for (int j = 0; j < k; ++j)
      if ((*all)[j] == (*all)[k])
        return batch_fail(lead, 2 * n, CVH_ERR_ARG, "%s: member %d: context %c is also member %d's context %c (every context may appear once)", what, k / 2, "ab"[k & 1],
                          j / 2, "ab"[j & 1]);
  unsigned long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    if (as[i]->device != as[0]->device)
      return batch_fail(lead, 2 * n, CVH_ERR_ARG, "%s: member %d is on device %d, member 0 on device %d", what, i, as[i]->device, as[0]->device);
    const int rc = pair_rules(lead, 2 * n, as[i], bs[i], what, member_prefix(i).c_str(), true);
    if (rc != CVH_OK) return rc;
    blocks += cvh_mp_geometry(as[i]->h, as[i]->w).grid;
    if (blocks >= (1ull << 31)) return batch_fail(lead, 2 * n, CVH_ERR_ARG, "%s: member %d: the members up to this one need 2^31 workgroups or more in one launch", what, i);
  }
  return CVH_OK;
}

// the contexts of n pairs (all = [A0, B0, A1, B1, ...]) settled, their FP64 mirrors fresh, every A's workspace there
int pairs_ready(cvh_context *const *all, int n, const char *what, const CvhMpGeom *g)
{
  HIPCHK(all[0], hipSetDevice(all[0]->device));
  int rc = settle_all(all, 2 * n, what);
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(all, 2 * n, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *a = all[2 * i];
    const size_t bytes = kMpStateBytes + (size_t)g[i].nitems * cvh_mp_nsums(a->C) * sizeof(double);
    rc = ensure_workspace(a, &a->d_multiphase, bytes, "multiphase", false);
    if (rc != CVH_OK) return batch_fail(all, 2 * n, rc, "%s: %s", what, a->err);
  }
  return CVH_OK;
}

// everything of a pair's record but the state slot, the trace and the prefix block count; u[0][e] is the buffer that holds the level set now
void pair_args(cvh_context *const *ctxs, const CvhMpGeom &g, CvhMpArgs *m)
{
  const cvh_context *a = ctxs[0];
  memset(m, 0, sizeof(*m));
  for (int k = 0; k < a->C; ++k) m->img[k] = a->d_img[k];
  m->st = (CvhMpState *)a->d_multiphase;
  m->partials = (double *)((unsigned char *)a->d_multiphase + kMpStateBytes);
  m->h = a->h; m->w = a->w;
  m->g = g;
  for (int e = 0; e < 2; ++e) {
    const cvh_context *c = ctxs[e];
    const int cur = current_buffer(c);
    m->u[0][e] = c->d_u[cur]; m->u[1][e] = c->d_u[cur ^ 1];
    m->alpha[e] = c->p.mu * c->p.dt;          // the addWeighted form of src/main.cpp:985, as fill_args (csv_run.hip)
    m->beta[e] = (1.0 / c->C) * c->p.dt;
    m->gamma[e] = -c->p.nu * c->p.dt;
    for (int k = 0; k < c->C; ++k) { m->lambda1[e][k] = c->p.lambda1[k]; m->lambda2[e][k] = c->p.lambda2[k]; }
    m->stop[e] = c->p.tol * c->stop_norm;
  }
  fill_front_args(a, &m->f);
}

// the sections of a class's step grid: record r owns its pair's own grid behind those of the records of its class before it
void pairs_lay_out(CvhMpArgs *recs, MarchClass *cls)
{
  for (int k = 0; k < kMarchClasses; ++k) {
    unsigned first = 0;
    for (int r = cls[k].first; r < cls[k].first + cls[k].n; ++r) { recs[r].first = first; first += recs[r].g.grid; }
    cls[k].grid = first;
  }
}

// one launch per kernel and class present, on the leader's stream.  init: the sums of the current pairs (parity 0) and the means they
// give into the state blocks; else one iteration of parity `parity`.  one: the call's only record on the host, which then travels by value
int pairs_launches(cvh_context *lead, const CvhMpArgs *d_recs, const MarchClass *cls, int parity, bool init, const CvhMpArgs *one)
{
  for (int k = 0; k < kMarchClasses; ++k) {
    const MarchClass &q = cls[k];
    if (!q.n) continue;
    const CvhMpArgs *tab = d_recs + q.first;
    if (init) HIPCHK(lead, cvh_launch_mp_sums(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one));
    else HIPCHK(lead, cvh_launch_mp_step(tab, q.n, q.grid, parity, q.C, q.fast, lead->stream, one));
    HIPCHK(lead, cvh_launch_mp_finalize(tab, q.n, q.C, init ? 1 : 0, lead->stream, one));
  }
  return CVH_OK;
}

// all = [A0, B0, A1, B1, ...] has passed pair_check (one pair) or pairs_batch_check; who(k) opens what a message says about context all[k]
int multiphase_run(cvh_context *const *all, int n, int max_steps, int *steps_done, double *norms, double *const *traces, int trace_rows, int *rows,
                   const char *what, const std::function<std::string(int)> &who)
{
  cvh_context *lead = all[0];
  MarchRun run{all, n, 2, what, who};
  int rc = run.begin(max_steps, traces, trace_rows, rows);
  if (rc != CVH_OK) return rc;
  std::vector<CvhMpGeom> g((size_t)n);
  for (int i = 0; i < n; ++i) g[i] = cvh_mp_geometry(all[2 * i]->h, all[2 * i]->w);
  rc = pairs_ready(all, n, what, g.data());
  if (rc != CVH_OK) return rc;
  for (int k = 0; k < 2 * n; ++k) {   // the stop norms (taken again where the planes changed on the device)
    rc = prepare_host(all[k]);
    if (rc != CVH_OK) return batch_fail(all, 2 * n, rc, "%s: %s%s", what, who(k).c_str(), all[k]->err);
  }
  rc = run.open([&](int i) { return &all[2 * i]->mp_trace; }, [&](int i) { return 4 * all[2 * i]->C + 2; }, sizeof(CvhMpArgs), kMpSlotBytes);
  if (rc != CVH_OK) return rc;
  std::vector<int> order;
  MarchClass cls[kMarchClasses];
  march_classes(all, n, 2, &order, cls);
  CvhMpArgs *recs = (CvhMpArgs *)run.record(0);
  for (int r = 0; r < n; ++r) {
    const int i = order[r];
    pair_args(all + 2 * i, g[i], &recs[r]);
    recs[r].st_mirror = (CvhMpState *)run.d_state(i);
    recs[r].trace = run.d_trace[i]; recs[r].trace_cap = run.trace_cap[i];
  }
  pairs_lay_out(recs, cls);
  // ONE pair: its record travels by value -- u[0][e] read, u[1][e] written, swapped here per iteration -- nothing is uploaded, and the
  // host reads the pair's own state block: the single call's launches as they were before the batch existed
  CvhMpArgs *one = n == 1 ? recs : nullptr;
  double *const bufs[2][2] = {{recs[0].u[0][0], recs[0].u[0][1]}, {recs[0].u[1][0], recs[0].u[1][1]}};   // [parity][level set]
  if (one) run.own_state = all[0]->d_multiphase;
  else rc = run.upload();
  if (rc != CVH_OK) return rc;
  const CvhMpArgs *d_recs = (const CvhMpArgs *)run.d_record(0);
  rc = pairs_launches(lead, d_recs, cls, 0, true, one);   // (its finalise writes the whole state block: where the localised flow zeroes its own)
  if (rc != CVH_OK) return rc;
  rc = run.iterate([&](int parity) {
    for (int e = 0; one && e < 2; ++e) { one->u[0][e] = bufs[parity][e]; one->u[1][e] = bufs[parity ^ 1][e]; }
    return pairs_launches(lead, d_recs, cls, parity, false, one);
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const CvhMpState *st = (const CvhMpState *)run.state(i);
    if (steps_done) steps_done[i] = st->run.steps_done;
    if (norms) { norms[2 * i] = st->norm[0]; norms[2 * i + 1] = st->norm[1]; }
  }
  return CVH_OK;
}

int multiphase_means(cvh_context *a, cvh_context *b, double *c, const char *what)
{
  cvh_context *ctxs[2];
  int rc = pair_check(a, b, what, true, ctxs);
  if (rc != CVH_OK) return rc;
  if (!c) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: c is NULL", what);
  const CvhMpGeom g = cvh_mp_geometry(a->h, a->w);
  rc = pairs_ready(ctxs, 1, what, &g);
  if (rc != CVH_OK) return rc;
  CvhMpArgs m;   // one record, by value
  pair_args(ctxs, g, &m);
  MarchClass cls[kMarchClasses];
  std::vector<int> order;
  march_classes(ctxs, 1, 2, &order, cls);
  pairs_lay_out(&m, cls);
  rc = open_call(ctxs, 2, nullptr);
  if (rc != CVH_OK) return rc;
  rc = pairs_launches(a, nullptr, cls, 0, true, &m);
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
    return multiphase_run(ctxs, 1, max_steps, steps_done, norms, traces, trace_rows, rows, what,
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
    return multiphase_run(all.data(), n, max_steps, steps_done, norms, traces, trace_rows, rows, what,
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

extern "C" void cvh_multiphase_geometry(int h, int w, int *cols, int *strip_rows, int *items)
{
  CvhMpGeom g{0, 0, 0, 0, 0};
  if (h > 0 && w > 0 && (long long)h * w < (1ll << 28)) g = cvh_mp_geometry(h, w);
  if (cols) *cols = CVH_MARCH_COLS;
  if (strip_rows) *strip_rows = g.strip_rows;
  if (items) *items = g.nitems;
}
