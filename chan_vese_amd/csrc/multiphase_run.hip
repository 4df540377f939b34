// multiphase_run.hip — host side of the four-phase calls (include/chanvese_hip.h, "Four phases"): two contexts A and B hold phi1 and
// phi2 of a Vese-Chan pair and are iterated together by multiphase_kernels.hip.  The pair has no object of its own: a call checks the
// pair, settles both contexts as the getters do and takes the pair's initial sums itself; cvh_multiphase_run then hands the iterations
// to march_run.hip's driver.  Per iteration two launches on A's stream: the step kernel (the update of both level sets and the items'
// partial sums of the new pair) and the one-workgroup finalise (means, norms, trace row, count, stop flag into the state block of A's
// workspace).
#include "cvh_host.h"

namespace {

constexpr size_t kMpStateBytes = 256;   // the workspace: [CvhMpState][the items' rows of partial sums]
static_assert(sizeof(CvhMpState) <= kMpStateBytes, "the workspace's first section holds the pair's state block");
static_assert(sizeof(CvhMpState) <= 4 * sizeof(CvhState), "the state block comes down into the context's pinned state slots");

// What every call refuses before anything is touched; ctxs[2] = {a, b} is filled here
int pair_check(cvh_context *a, cvh_context *b, const char *what, bool need_images, cvh_context **ctxs)
{
  ctxs[0] = a; ctxs[1] = b;
  if (!a || !b) return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: context %s is NULL", what, a ? "b" : "a");
  if (a == b) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: a and b are the same context (a pair is two contexts)", what);
  if (a->device != b->device) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: a is on device %d, b on device %d", what, a->device, b->device);
  if (a->h != b->h || a->w != b->w) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: a is %d x %d, b %d x %d", what, a->h, a->w, b->h, b->w);
  if (a->C != b->C) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: a has %d channel(s), b %d", what, a->C, b->C);
  if (a->p.eps != b->p.eps) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: eps must be equal in both contexts, got %g and %g", what, a->p.eps, b->p.eps);
  for (int i = 0; i < 2; ++i)
    if (ctxs[i]->state_bits == 32) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: context %c has \"state\" = 32: the pair iterates FP64 level sets", what, "ab"[i]);
  if (a->n >= ((size_t)1 << 28)) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: %d x %d is too large, h * w must stay below 2^28", what, a->h, a->w);
  for (int i = 0; i < 2; ++i) {
    if (need_images && !ctxs[i]->have_image)
      return batch_fail(ctxs, 2, CVH_ERR_STATE, "%s: context %c has no image (call cvh_set_image first)", what, "ab"[i]);
    if (!ctxs[i]->have_u) return batch_fail(ctxs, 2, CVH_ERR_STATE, "%s: context %c has no level set", what, "ab"[i]);
  }
  return CVH_OK;
}

// both contexts settled, their FP64 mirrors fresh, A's workspace there
int pair_ready(cvh_context *const *ctxs, const char *what, const CvhMpGeom &g)
{
  cvh_context *a = ctxs[0];
  HIPCHK(a, hipSetDevice(a->device));
  int rc = settle_all(ctxs, 2, what);
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(ctxs, 2, what);
  if (rc != CVH_OK) return rc;
  const size_t bytes = kMpStateBytes + (size_t)g.nitems * cvh_mp_nsums(a->C) * sizeof(double);
  rc = ensure_workspace(a, &a->d_multiphase, bytes, "multiphase", false);
  if (rc != CVH_OK) return batch_fail(ctxs, 2, rc, "%s: %s", what, a->err);
  return CVH_OK;
}

// everything of the launch arguments but in[] / out[] and the trace
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
    m->alpha[e] = c->p.mu * c->p.dt;          // the addWeighted form of src/main.cpp:985, as fill_args (csv_run.hip)
    m->beta[e] = (1.0 / c->C) * c->p.dt;
    m->gamma[e] = -c->p.nu * c->p.dt;
    for (int k = 0; k < c->C; ++k) { m->lambda1[e][k] = c->p.lambda1[k]; m->lambda2[e][k] = c->p.lambda2[k]; }
    m->stop[e] = c->p.tol * c->stop_norm;
  }
  fill_front_args(a, &m->f);
}

// the sums of the current pair and the means they give, into the state block, on A's stream
int initial_sums(cvh_context *const *ctxs, CvhMpArgs *m)
{
  cvh_context *a = ctxs[0];
  for (int e = 0; e < 2; ++e) { m->in[e] = ctxs[e]->d_u[current_buffer(ctxs[e])]; m->out[e] = nullptr; }
  HIPCHK(a, cvh_launch_mp_sums(*m, a->C, use_fast(a), a->stream));
  HIPCHK(a, cvh_launch_mp_finalize(*m, a->C, 1, a->stream));
  return CVH_OK;
}

int multiphase_run(cvh_context *a, cvh_context *b, int max_steps, int *steps_done, double *norms, double *trace, int trace_rows, int *rows,
                   const char *what)
{
  cvh_context *ctxs[2];
  int rc = pair_check(a, b, what, true, ctxs);
  if (rc != CVH_OK) return rc;
  MarchRun run{ctxs, 2, what, "ab"};
  rc = run.begin(max_steps, trace, trace_rows, rows);
  if (rc != CVH_OK) return rc;
  const CvhMpGeom g = cvh_mp_geometry(a->h, a->w);
  rc = pair_ready(ctxs, what, g);
  if (rc != CVH_OK) return rc;
  for (int e = 0; e < 2; ++e) {   // the stop norms (taken again where the planes changed on the device)
    rc = prepare_host(ctxs[e]);
    if (rc != CVH_OK) return batch_fail(ctxs, 2, rc, "%s: context %c: %s", what, "ab"[e], ctxs[e]->err);
  }
  const int C = a->C, fast = use_fast(a);
  rc = run.open(&a->mp_trace, 4 * C + 2);
  if (rc != CVH_OK) return rc;
  CvhMpArgs m;
  pair_args(ctxs, g, &m);
  m.trace = run.d_trace; m.trace_cap = run.trace_cap;
  rc = initial_sums(ctxs, &m);   // (its finalise writes the whole state block: where the localised flow zeroes its own)
  if (rc != CVH_OK) return rc;
  CvhMpState st;
  rc = run.iterate(a->d_multiphase, &st, sizeof(st), [&](const double *const *in, double *const *out) -> int {
    for (int e = 0; e < 2; ++e) { m.in[e] = in[e]; m.out[e] = out[e]; }
    HIPCHK(a, cvh_launch_mp_step(m, C, fast, a->stream));
    HIPCHK(a, cvh_launch_mp_finalize(m, C, 0, a->stream));
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  if (steps_done) *steps_done = st.run.steps_done;
  if (norms) { norms[0] = st.norm[0]; norms[1] = st.norm[1]; }
  return CVH_OK;
}

int multiphase_means(cvh_context *a, cvh_context *b, double *c, const char *what)
{
  cvh_context *ctxs[2];
  int rc = pair_check(a, b, what, true, ctxs);
  if (rc != CVH_OK) return rc;
  if (!c) return batch_fail(ctxs, 2, CVH_ERR_ARG, "%s: c is NULL", what);
  const CvhMpGeom g = cvh_mp_geometry(a->h, a->w);
  rc = pair_ready(ctxs, what, g);
  if (rc != CVH_OK) return rc;
  CvhMpArgs m;
  pair_args(ctxs, g, &m);
  rc = open_call(ctxs, 2, nullptr);
  if (rc != CVH_OK) return rc;
  rc = initial_sums(ctxs, &m);
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
  return guarded(nullptr, 0, what, [&]() { return multiphase_run(a, b, max_steps, steps_done, norms, trace, trace_rows, rows, what); });
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
