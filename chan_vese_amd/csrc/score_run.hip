// score_run.hip — host side of the mask scores (include/chanvese_hip.h, "Mask scores"): the masks of n contexts against ground-truth
// planes, as the integers of cvh_mask_score.  One MemberCall (cvh_host.h, io_run.hip: member tables, stream joins, event ordering against
// the caller's stream, the one host wait) around score_kernels.hip's four launches; the single forms are batches of one, and the host
// form stages its bytes into the context's workspace on the context's stream and is then the device form on that stream.  The calls only
// read: the members are settled and their FP64 mirrors refreshed as the getters do, and nothing of a member's run state is assigned here.
#include "cvh_host.h"

namespace {

int score_batch(cvh_context *const *ctxs, int n, const uint8_t *const *d_truths, int invert, uint32_t tol2, cvh_mask_score *out, void *stream,
                const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  if (!out) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: out is NULL", what);
  if (!d_truths) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of device pointers is NULL", what);
  rc = members_below(ctxs, n, what, 31);
  if (rc == CVH_OK) rc = members_distances_fit(ctxs, n, what);   // (the passes are cvh_reinit's)
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; i < n; ++i) { rc = pointer_check(ctxs, n, i, d_truths[i], what); if (rc != CVH_OK) return rc; }
  rc = members_have_levelsets(ctxs, n, what);   // (the arguments first, then the members' state: as the getters)
  if (rc != CVH_OK) return rc;
  rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    rc = ensure_workspace(c, &c->d_score, cvh_score_workspace_bytes(c->h, c->w), "score");
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, c->err);
  }
  // staging: [column-pass table][row-pass table][one result row per member, zero]
  const size_t row_bytes = (size_t)n * CVH_SCORE_ROW * sizeof(unsigned long long);
  MemberCall call;
  rc = call.begin(ctxs, n, what, row_bytes, 0, true);
  if (rc != CVH_OK) return rc;
  unsigned long long *const rows = (unsigned long long *)(call.hb + call.extra_off);
  int max_w = 0;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    CvhIoMember &m = call.tab[i];
    m.src = c->d_u[current_buffer(c)];
    m.src2 = d_truths[i];
    m.plane[0] = (uint8_t *)c->d_score;
    m.plane[1] = (uint8_t *)c->d_score + 4 * cvh_score_words_bytes(c->h, c->w);
    m.sums = (unsigned long long *)(call.db + call.extra_off) + (size_t)CVH_SCORE_ROW * i;
    call.tab2[i] = m;
    m.nblk = cvh_reinit_column_blocks(c->h, c->w);
    call.tab2[i].nblk = cvh_reinit_row_blocks(c->h);
    max_w = std::max(max_w, c->w);
  }
  rc = call.run(stream, false, true, [&]() -> int {   // the ONE host wait of the call: the result rows
    HIPCHK(lead, cvh_launch_score(call.dtab(), call.grid, call.dtab2(), call.grid2, n, max_w, invert, tol2, lead->stream));
    ++g_launches[kScoreLaunchSets];
    HIPCHK(lead, hipMemcpyAsync(rows, call.db + call.extra_off, row_bytes, hipMemcpyDeviceToHost, lead->stream));
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const unsigned long long *r = rows + (size_t)CVH_SCORE_ROW * i;
    cvh_mask_score &s = out[i];
    memset(&s, 0, sizeof(s));
    s.tp = r[CVH_SCORE_TP]; s.fp = r[CVH_SCORE_FP]; s.fn = r[CVH_SCORE_FN]; s.tn = r[CVH_SCORE_TN];
    s.surf_m = r[CVH_SCORE_SURF_M]; s.surf_t = r[CVH_SCORE_SURF_T];
    s.defined = s.surf_m != 0 && s.surf_t != 0;
    if (!s.defined) continue;   // (launches 3 and 4 returned at once: the six fields are the zeros of the cleared row)
    s.within_m = r[CVH_SCORE_WITHIN_M]; s.within_t = r[CVH_SCORE_WITHIN_T];
    s.dist_m_q16 = r[CVH_SCORE_DIST_M]; s.dist_t_q16 = r[CVH_SCORE_DIST_T];
    s.hd2_m = (uint32_t)r[CVH_SCORE_HD2_M]; s.hd2_t = (uint32_t)r[CVH_SCORE_HD2_T];
  }
  return CVH_OK;
}

}  // namespace

extern "C" int cvh_score_mask_device_batch(cvh_context *const *ctxs, int n, const uint8_t *const *d_truths, int invert, uint32_t tol2,
                                           cvh_mask_score *out, void *stream)
{
  static const char what[] = "cvh_score_mask_device_batch";
  return guarded(ctxs, n, what, [&]() { return score_batch(ctxs, n, d_truths, invert, tol2, out, stream, what); });
}

extern "C" int cvh_score_mask_device(cvh_context *c, const uint8_t *d_truth, int invert, uint32_t tol2, cvh_mask_score *out, void *stream)
{
  return guarded_one(c, "cvh_score_mask_device", [&](const char *what) { return score_batch(&c, 1, &d_truth, invert, tol2, out, stream, what); });
}

extern "C" int cvh_score_mask(cvh_context *c, const uint8_t *truth, int invert, uint32_t tol2, cvh_mask_score *out)
{
  return guarded_one(c, "cvh_score_mask", [&](const char *what) {
    if (!truth) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: truth is NULL", what);
    if (!out) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: out is NULL", what);
    if (c->n >= ((size_t)1 << 31)) return members_below(&c, 1, what, 31);
    if (!c->have_u) return members_have_levelsets(&c, 1, what);   // before the workspace is allocated
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_workspace(c, &c->d_score, cvh_score_workspace_bytes(c->h, c->w), "score", false);
    if (rc != CVH_OK) return batch_fail(&c, 1, rc, "%s: %s", what, std::string(c->err).c_str());
    // the bytes ride the context's stream (idle or not: the workspace's truth plane is read by this call's launches alone, which the
    // same stream orders behind the copy and, by the call's host wait, in front of the next call's copy)
    uint8_t *staged = (uint8_t *)c->d_score + cvh_score_truth_offset(c->h, c->w);
    HIPCHK(c, hipMemcpyAsync(staged, truth, c->n, hipMemcpyHostToDevice, c->stream));
    const uint8_t *d_truth = staged;
    return score_batch(&c, 1, &d_truth, invert, tol2, out, c->stream, what);
  });
}
