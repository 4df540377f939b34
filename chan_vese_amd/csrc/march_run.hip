// march_run.hip — the host driver under the marching-wave calls: cvh_multiphase_run[_batch], cvh_localized_run[_batch],
// cvh_geodesic_run[_batch] and cvh_convex_run[_batch] (MarchRun, cvh_host.h; the call sequence around it, written once over a flow description, is march_flow.h's).
// The level sets of N members (contexts, or pairs of contexts) are iterated together on the leader's stream; a single call is a batch
// of one member.
// Data flow: the leader's table holds one argument record per member -- both buffers of every level set in it -- and one state slot
// per member; it is uploaded once per call.  Iteration t reads d_u[(current + t) & 1] of each context and writes the other buffer of
// its pair -- the contexts' own ping-pong pairs; the parity t & 1 is a kernel argument -- with no copy of a level set but at most ONE
// at the end, where the member's last iteration's buffer is not the one a new level set lands in.  A member's finalise workgroup
// writes the member's own state block and mirrors it in its slot of the table.  The host enqueues the leader's "sync_every" iterations
// at a time and copies the state slots down behind each chunk: one copy and one wait per chunk, whatever N.  Launches enqueued behind
// a member's stop return at once for that member (every workgroup reads its member's flag), so its level set stays as its stopping
// iteration left it and the host picks the buffers by the parity of the member's steps_done.  A run ends with every context exactly as
// a device-side start leaves it: the level set in the buffer cvh_set_levelset writes, the device's half of a new run done on the
// leader's stream, then levelset_arrived -- every existing call sees the new level sets.
// A call with ONE member keeps the single call's launches as they were before the batch existed (own_state): its record travels by
// value, the caller swaps the two buffers in it between iterations, nothing is uploaded, no mirror is written, and the member's own
// state block comes down behind a chunk.
#include "cvh_host.h"

// the FAST forms' constants; the values fill_args (csv_run.hip) computes into CvhStepArgs, whose layout keeps them apart
void fill_front_args(const cvh_context *c, CvhFrontArgs *f)
{
  const double pi = 3.14159265358979323846;
  f->eps = c->p.eps;
  f->inv_eps = 1.0 / c->p.eps;
  f->dk1 = pi / c->p.eps;
  far_coef(c->p.eps, c->far_terms, f->far_k, &f->far_thr);
  f->atan2_tab = c->d_atan + 2 * CVH_ATAN_N;
}

std::string member_prefix(int i) { return "member " + std::to_string(i) + ": "; }

int state_down(cvh_context *a, const void *d_state, void *out, size_t bytes)
{
  HIPCHK(a, hipMemcpyAsync(a->h_state, d_state, bytes, hipMemcpyDeviceToHost, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  memcpy(out, a->h_state, bytes);
  return CVH_OK;
}

int march_stage(cvh_context *lead, size_t dev_bytes, size_t host_bytes, unsigned char **h, unsigned char **d)
{
  if (lead->h_march_cap < host_bytes) {
    if (lead->h_march) { HIPCHK(lead, hipHostFree(lead->h_march)); lead->h_march = nullptr; lead->h_march_cap = 0; }
    const size_t cap = align_up(host_bytes + host_bytes / 4, 4096);
    HIPCHK(lead, hipHostMalloc(&lead->h_march, cap, hipHostMallocDefault));
    lead->h_march_cap = cap;
  }
  const int rc = grow_table(lead, &lead->march_table, dev_bytes);
  if (rc != CVH_OK) return rc;
  memset(lead->h_march, 0, host_bytes);
  *h = (unsigned char *)lead->h_march;
  *d = (unsigned char *)lead->march_table.d;
  return CVH_OK;
}

// the folded parameters of one level set's equation, as fill_args (csv_run.hip): the addWeighted form of src/main.cpp:985
void march_params(const cvh_context *c, double *alpha, double *beta, double *gamma, double *lambda1, double *lambda2, double *stop)
{
  *alpha = c->p.mu * c->p.dt;
  *beta = (1.0 / c->C) * c->p.dt;
  *gamma = -c->p.nu * c->p.dt;
  for (int k = 0; k < c->C; ++k) { lambda1[k] = c->p.lambda1[k]; lambda2[k] = c->p.lambda2[k]; }
  *stop = c->p.tol * c->stop_norm;
}

int march_rules(cvh_context *const *lead, int nlead, cvh_context *const *m, int per, const char *what, const char *who, bool need_images)
{
  auto noun = [&](int e) { return per == 1 ? std::string("the context") : std::string("context ") + "ab"[e]; };
  for (int e = 0; e < per; ++e)
    if (m[e]->state_bits == 32)
      return batch_fail(lead, nlead, CVH_ERR_ARG, "%s: %s%s has \"state\" = 32: %s", what, who, noun(e).c_str(),
                        per == 1 ? "the call iterates an FP64 level set" : "the pair iterates FP64 level sets");
  if (m[0]->n >= ((size_t)1 << 28)) return batch_fail(lead, nlead, CVH_ERR_ARG, "%s: %s%d x %d is too large, h * w must stay below 2^28", what, who, m[0]->h, m[0]->w);
  for (int e = 0; e < per; ++e) {
    if (need_images && !m[e]->have_image)
      return batch_fail(lead, nlead, CVH_ERR_STATE, "%s: %s%s has no image (call cvh_set_image first)", what, who, noun(e).c_str());
    if (!m[e]->have_u) return batch_fail(lead, nlead, CVH_ERR_STATE, "%s: %s%s has no level set", what, who, noun(e).c_str());
  }
  return CVH_OK;
}

void march_strip_geometry(int h, int w, int *cols, int *strip_rows, int *items)
{
  CvhMpGeom g{0, 0, 0, 0, 0};
  if (h > 0 && w > 0 && (long long)h * w < (1ll << 28)) g = cvh_mp_geometry(h, w);
  if (cols) *cols = CVH_MARCH_COLS;
  if (strip_rows) *strip_rows = g.strip_rows;
  if (items) *items = g.nitems;
}

int MarchRun::begin(int max_steps_, double *const *traces_, int trace_rows_, int *rows_)
{
  bool any = false;
  for (int i = 0; traces_ && i < n; ++i) any = any || traces_[i];
  if (any && (trace_rows_ < 0 || !rows_))
    return batch_fail(ctxs, n * per, CVH_ERR_ARG, "%s: a trace needs trace_rows >= 0 and rows, got trace_rows = %d, rows = %p", what, trace_rows_, (void *)rows_);
  max_steps = max_steps_ < 0 ? INT_MAX : max_steps_;   // (as cvh_run: until the stop rule fires)
  traces = any ? traces_ : nullptr; trace_rows = trace_rows_; rows = rows_;
  trace_cap.assign((size_t)n, 0);
  for (int i = 0; traces && i < n; ++i) trace_cap[i] = traces[i] ? std::min(trace_rows, max_steps) : 0;
  return CVH_OK;
}

// (open_call / close_call only order streams -- the leader's behind every member's, and back -- and hold nothing: a HIP error between
// them leaves no call open; what such an error does leave is the header's "partly iterated" level set)
int MarchRun::open(const std::function<DeviceTable *(int)> &table_of, const std::function<int(int)> &width_of, size_t rec_size_, size_t state_stride_)
{
  cvh_context *lead = ctxs[0];
  d_trace.assign((size_t)n, nullptr);
  row_width.assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    row_width[i] = width_of(i);
    if (trace_cap[i] <= 0) continue;
    cvh_context *owner = ctxs[(size_t)i * per];
    DeviceTable *t = table_of(i);
    const int rc = grow_table(owner, t, (size_t)trace_cap[i] * row_width[i] * sizeof(double));
    if (rc != CVH_OK) return batch_fail(ctxs, n * per, rc, "%s: %s%s", what, who(i * per).c_str(), owner->err);
    d_trace[i] = (double *)t->d;
  }
  rec_size = rec_size_; state_stride = state_stride_;
  state_off = align_up((size_t)n * rec_size, 256);
  dev_bytes = state_off + (size_t)n * state_stride;
  land_off = align_up(dev_bytes, 256);
  const int rc = march_stage(lead, dev_bytes, land_off + (size_t)n * state_stride, &h_tab, &d_tab);
  if (rc != CVH_OK) return batch_fail(ctxs, n * per, rc, "%s: %s", what, lead->err);
  cur.assign((size_t)n * per, 0);
  for (int k = 0; k < n * per; ++k) cur[k] = current_buffer(ctxs[k]);
  return open_call(ctxs, n * per, nullptr);
}

int MarchRun::upload()
{
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipMemcpyAsync(d_tab, h_tab, dev_bytes, hipMemcpyHostToDevice, lead->stream));   // (the state slots: zeros)
  return CVH_OK;
}

int MarchRun::iterate(const std::function<int(int parity)> &step)
{
  cvh_context *a = ctxs[0];
  auto count = [&](int i) { return (const CvhMarchCount *)state(i); };
  auto all_stopped = [&]() {
    for (int i = 0; i < n; ++i)
      if (!count(i)->stopped) return false;
    return true;
  };
  HIPCHK(a, hipEventRecord(a->ev0, a->stream));   // (ev0 / ev1 are free: settle closed any timed run)
  int enq = 0;
  while (enq < max_steps && !all_stopped()) {
    const int chunk = std::min(a->sync_every, max_steps - enq);
    for (int t = enq; t < enq + chunk; ++t) {
      const int rc = step(t & 1);
      if (rc != CVH_OK) return rc;
    }
    enq += chunk;
    HIPCHK(a, hipEventRecord(a->ev1, a->stream));
    HIPCHK(a, hipMemcpyAsync(h_tab + land_off, own_state ? own_state : d_tab + state_off, (size_t)n * state_stride, hipMemcpyDeviceToHost, a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));   // the ONE host wait of the chunk
  }
  if (enq > 0) HIPCHK(a, hipEventElapsedTime(&a->last_run_ms, a->ev0, a->ev1));
  // each level set of its member's iteration steps_done - 1 into the buffer a new level set lands in, and the device's half of the run it begins
  std::vector<int> nrows((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    const int done = count(i)->steps_done;
    for (int e = 0; e < per; ++e) {
      cvh_context *c = ctxs[(size_t)i * per + e];
      const int from = (cur[(size_t)i * per + e] + done) & 1, to = c->chain_pb & 1;
      if (bake) { const int rc = bake(i * per + e, done); if (rc != CVH_OK) return rc; }
      else if (from != to) HIPCHK(a, hipMemcpyAsync(c->d_u[to], c->d_u[from], c->n * sizeof(double), hipMemcpyDeviceToDevice, a->stream));
      HIPCHK(a, clear_run_device(c, a->stream));
    }
    nrows[i] = std::min(done, trace_cap[i]);
    if (nrows[i] > 0)
      HIPCHK(a, hipMemcpyAsync(traces[i], d_trace[i], (size_t)nrows[i] * row_width[i] * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  }
  int rc = close_call(ctxs, n * per, nullptr, false);
  if (rc != CVH_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(a->stream));
  for (int k = 0; k < n * per; ++k) {
    rc = levelset_arrived(ctxs[k], true);
    if (rc != CVH_OK) return batch_fail(ctxs, n * per, rc, "%s: %s%s", what, who(k).c_str(), ctxs[k]->err);
  }
  for (int i = 0; rows && i < n; ++i) rows[i] = nrows[i];
  return CVH_OK;
}
