// march_run.hip — the host driver under cvh_multiphase_run and cvh_localized_run (MarchRun, cvh_host.h): the level sets of N contexts are
// iterated together on the leader's stream.  Data flow: iteration t reads d_u[(current + t) & 1] of each context and writes the other
// buffer of its pair -- the contexts' own ping-pong pairs, no copy of a level set but at most ONE at the end, where the last iteration's
// buffer is not the one a new level set lands in.  The host enqueues the leader's "sync_every" iterations at a time and reads the state
// block behind each chunk: its only wait per chunk.  Launches enqueued behind a stop return at once (every workgroup reads the flag), so
// the level sets stay as the stopping iteration left them and the host picks the buffers by the parity of steps_done.  A run ends with
// every context exactly as a device-side start leaves it: the level set in the buffer cvh_set_levelset writes, the device's half of a
// new run done on the leader's stream, then levelset_arrived -- every existing call sees the new level sets.
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

int state_down(cvh_context *a, const void *d_state, void *out, size_t bytes)
{
  HIPCHK(a, hipMemcpyAsync(a->h_state, d_state, bytes, hipMemcpyDeviceToHost, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  memcpy(out, a->h_state, bytes);
  return CVH_OK;
}

int MarchRun::begin(int max_steps_, double *trace_, int trace_rows, int *rows_)
{
  if (trace_ && (trace_rows < 0 || !rows_))
    return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: a trace needs trace_rows >= 0 and rows, got trace_rows = %d, rows = %p", what, trace_rows, (void *)rows_);
  max_steps = max_steps_ < 0 ? INT_MAX : max_steps_;   // (as cvh_run: until the stop rule fires)
  trace = trace_; rows = rows_;
  trace_cap = trace ? std::min(trace_rows, max_steps) : 0;
  return CVH_OK;
}

// (open_call / close_call only order streams -- the leader's behind the legacy stream, and back -- and hold nothing: a HIP error between
// them leaves no call open; what such an error does leave is the header's "partly iterated" level set)
int MarchRun::open(DeviceTable *table_, int row_width_)
{
  cvh_context *a = ctxs[0];
  table = table_; row_width = row_width_;
  if (trace_cap > 0) {
    const int rc = grow_table(a, table, (size_t)trace_cap * row_width * sizeof(double));
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: %s", what, a->err);
    d_trace = (double *)table->d;
  }
  return open_call(ctxs, n, nullptr);
}

int MarchRun::iterate(const void *d_state, void *st, size_t state_bytes, const std::function<int(const double *const *in, double *const *out)> &step)
{
  cvh_context *a = ctxs[0];
  const CvhMarchCount *count = (const CvhMarchCount *)st;
  int cur[2] = {0, 0};
  for (int e = 0; e < n; ++e) cur[e] = current_buffer(ctxs[e]);
  memset(st, 0, state_bytes);
  HIPCHK(a, hipEventRecord(a->ev0, a->stream));   // (ev0 / ev1 are free: settle closed any timed run)
  int enq = 0;
  while (enq < max_steps && !count->stopped) {
    const int chunk = std::min(a->sync_every, max_steps - enq);
    for (int t = enq; t < enq + chunk; ++t) {
      const double *in[2] = {nullptr, nullptr};
      double *out[2] = {nullptr, nullptr};
      for (int e = 0; e < n; ++e) { in[e] = ctxs[e]->d_u[(cur[e] + t) & 1]; out[e] = ctxs[e]->d_u[(cur[e] + t + 1) & 1]; }
      const int rc = step(in, out);
      if (rc != CVH_OK) return rc;
    }
    enq += chunk;
    HIPCHK(a, hipEventRecord(a->ev1, a->stream));
    const int rc = state_down(a, d_state, st, state_bytes);   // the ONE host wait of the chunk
    if (rc != CVH_OK) return rc;
  }
  if (enq > 0) HIPCHK(a, hipEventElapsedTime(&a->last_run_ms, a->ev0, a->ev1));
  // the level sets of iteration steps_done - 1 into the buffers a new level set lands in, and the device's half of the run it begins
  for (int e = 0; e < n; ++e) {
    cvh_context *c = ctxs[e];
    const int from = (cur[e] + count->steps_done) & 1, to = c->chain_pb & 1;
    if (from != to) HIPCHK(a, hipMemcpyAsync(c->d_u[to], c->d_u[from], c->n * sizeof(double), hipMemcpyDeviceToDevice, a->stream));
    HIPCHK(a, clear_run_device(c, a->stream));
  }
  nrows = std::min(count->steps_done, trace_cap);
  if (nrows > 0) HIPCHK(a, hipMemcpyAsync(trace, table->d, (size_t)nrows * row_width * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  int rc = close_call(ctxs, n, nullptr, false);
  if (rc != CVH_OK) return rc;
  HIPCHK(a, hipStreamSynchronize(a->stream));
  for (int e = 0; e < n; ++e) {
    rc = levelset_arrived(ctxs[e], true);
    if (rc == CVH_OK) continue;
    if (n == 1) return batch_fail(ctxs, n, rc, "%s: %s", what, ctxs[e]->err);
    return batch_fail(ctxs, n, rc, "%s: context %c: %s", what, names[e], ctxs[e]->err);
  }
  if (rows) *rows = nrows;
  return CVH_OK;
}
