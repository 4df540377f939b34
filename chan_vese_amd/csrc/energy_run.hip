// energy_run.hip — host side of the energy calls (include/chanvese_hip.h, "Energy"): the terms of the Chan-Sandberg-Vese functional of
// the current level sets of n contexts.  One MemberCall (cvh_host.h, io_run.hip: member table, stream joins, event ordering, the one
// host wait) around energy_kernels.hip's two launches; the single form is a batch of one.  The calls only read: the members are
// settled and their FP64 mirrors refreshed as the getters do, and nothing of a member's run state is assigned here.
// Means: c1 / c2 are what cvh_get_means returns.  Where the member's state block holds the means of the current level set (prepare's own
// test, csv_run.hip) the term pass reads them there.  Where it does not, cvh_get_means would take them with csv_init_sums_kernel and
// csv_finalize_kernel; the same two kernels are enqueued here, in front of the term pass on the leader's stream, on the same level
// set, planes, eps and grid -- hence the same bits -- but they finalise into a CvhState of the member's energy workspace and are given
// no chain set to seed: the run's state block, its fixed-point sum sets and its validity flags stay as they were, and the run takes
// its sums itself when it goes on, as it would have without the call.
#include "cvh_host.h"

namespace {

// prepare()'s test (csv_run.hip): the state block does not hold the means cvh_get_means would return for the current level set
bool means_stale(const cvh_context *c)
{
  return !c->sums_valid || (use_chain(c, resolve_geometry(c)) && !c->chain_acc_valid);
}

// the arguments csv_init_sums_kernel and the initial csv_finalize_kernel read, with `st` in place of the context's state block
void init_sum_args(const cvh_context *c, CvhState *st, CvhStepArgs *a)
{
  memset(a, 0, sizeof(*a));
  a->u_in = c->d_u[current_buffer(c)];
  for (int k = 0; k < c->C; ++k) a->img[k] = c->d_img[k];
  a->h = c->h; a->w = c->w;
  a->eps = c->p.eps;
  a->partials = c->d_partials;   // idle: the member is settled, and the leader's stream is joined with the member's
  a->st = st;
}

int energy_batch(cvh_context *const *ctxs, int n, cvh_energy_terms *out, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  if (!out) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: out is NULL", what);
  rc = members_below(ctxs, n, what, 32);
  if (rc != CVH_OK) return rc;
  rc = members_have_images(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  rc = members_have_levelsets(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  constexpr size_t kStateBytes = 256;   // the workspace: [CvhState][item rows]
  static_assert(sizeof(CvhState) <= kStateBytes, "the workspace's first section holds a CvhState");
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    const size_t bytes = kStateBytes + (size_t)cvh_energy_items(c->h, c->w) * CVH_ENERGY_SLOTS * sizeof(double);
    rc = ensure_workspace(c, &c->d_energy, bytes, "energy", false);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, c->err);
  }
  // staging: [member table][one row of CVH_ENERGY_ROW doubles per member: eps up, the results down]
  const size_t row_bytes = (size_t)n * CVH_ENERGY_ROW * sizeof(double);
  MemberCall call;
  rc = call.begin(ctxs, n, what, row_bytes);
  if (rc != CVH_OK) return rc;
  double *const rows = (double *)(call.hb + call.extra_off);
  std::vector<int> stale((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    CvhIoMember &m = call.tab[i];
    stale[i] = means_stale(c);
    m.src = c->d_u[current_buffer(c)];
    m.src2 = stale[i] ? c->d_energy : (const void *)c->d_state;
    for (int k = 0; k < c->C; ++k) m.plane[k] = c->d_img[k];
    m.dst = (unsigned char *)c->d_energy + kStateBytes;
    m.sums = (unsigned long long *)(call.db + call.extra_off) + (size_t)CVH_ENERGY_ROW * i;
    m.nblk = cvh_energy_blocks(c->h, c->w);
    rows[(size_t)CVH_ENERGY_ROW * i] = c->p.eps;
  }
  rc = call.run(nullptr, false, true, [&]() -> int {   // the ONE host wait of the call: the terms
    for (int i = 0; i < n; ++i) {
      if (!stale[i]) continue;
      const cvh_context *c = ctxs[i];
      CvhStepArgs a;
      init_sum_args(c, (CvhState *)c->d_energy, &a);
      HIPCHK(lead, cvh_launch_init_sums(a, c->C, 0, &a.nparts, lead->stream));
      HIPCHK(lead, cvh_launch_finalize(a, c->C, 1, lead->stream));
    }
    HIPCHK(lead, cvh_launch_energy(call.dtab(), n, call.grid, lead->stream));
    ++g_launches[kEnergyLaunchSets];
    HIPCHK(lead, hipMemcpyAsync(rows, call.db + call.extra_off, row_bytes, hipMemcpyDeviceToHost, lead->stream));
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    const double *r = rows + (size_t)CVH_ENERGY_ROW * i;
    cvh_energy_terms &t = out[i];
    memset(&t, 0, sizeof(t));
    t.length = r[1];
    t.area = r[2];
    // total = mu length + nu area + (1/C) sum_k (lambda1_k fit_in[k] + lambda2_k fit_out[k]), left to right (no contraction: Makefile)
    double fit = 0.0;
    for (int k = 0; k < c->C; ++k) {
      t.fit_in[k] = r[3 + k];
      t.fit_out[k] = r[3 + CVH_MAX_CHANNELS + k];
      t.c1[k] = r[3 + 2 * CVH_MAX_CHANNELS + k];
      t.c2[k] = r[3 + 3 * CVH_MAX_CHANNELS + k];
      const double term = c->p.lambda1[k] * t.fit_in[k] + c->p.lambda2[k] * t.fit_out[k];
      fit = k ? fit + term : term;
    }
    t.total = c->p.mu * t.length + c->p.nu * t.area + (1.0 / c->C) * fit;
  }
  return CVH_OK;
}

}  // namespace

extern "C" int cvh_energy_batch(cvh_context *const *ctxs, int n, cvh_energy_terms *out)
{
  static const char what[] = "cvh_energy_batch";
  return guarded(ctxs, n, what, [&]() { return energy_batch(ctxs, n, out, what); });
}

extern "C" int cvh_energy(cvh_context *c, cvh_energy_terms *out)
{
  return guarded_one(c, "cvh_energy", [&](const char *what) { return energy_batch(&c, 1, out, what); });
}
