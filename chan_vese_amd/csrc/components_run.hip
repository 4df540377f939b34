// components_run.hip — host side of cvh_components* and cvh_get_mask_clean* (include/chanvese_hip.h, "Connected components"): read-only
// operations on the level sets of n contexts, each ONE MemberCall (cvh_host.h, io_run.hip: member table, stream joins, event ordering).
// The single-context calls are batches of one member (guarded_one); what the members must hold is asked of csv_batch.hip's predicates.
// Nothing here touches a context's level set, run state, sums or options.
#include "cvh_host.h"

namespace {

int conn_check(cvh_context *const *ctxs, int n, int conn, const char *what)
{
  if (conn != 4 && conn != 8) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: conn must be 4 or 8, got %d", what, conn);
  return CVH_OK;
}

// every member has a level set and a plane the 31-bit indices cover; iterations in flight are settled, the double mirror and the
// workspace exist
int members_ready(cvh_context *const *ctxs, int n, const char *what)
{
  int rc = members_below(ctxs, n, what, 31);
  if (rc == CVH_OK) rc = members_have_levelsets(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    rc = ensure_workspace(c, &c->d_cc, cvh_cc_workspace_bytes(c->n), "components");
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, c->err);
  }
  return CVH_OK;
}

// staging: [member table][a second one, if asked for: the caller's][one word per member, zero at extra_off][`more` bytes of the
// caller's, zero].  dst[i] is member i's output (may be null)
int fill_members(MemberCall *call, cvh_context *const *ctxs, int n, void *const *dst, const char *what, bool two_tables = false, size_t more = 0)
{
  const int rc = call->begin(ctxs, n, what, (size_t)n * sizeof(unsigned long long) + more, 0, two_tables);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    CvhIoMember &m = call->tab[i];
    m.src = c->d_u[current_buffer(c)];
    m.dst = dst ? dst[i] : nullptr;
    m.plane[0] = (uint8_t *)c->d_cc;
    m.plane[1] = m.plane[0] + c->n * sizeof(unsigned);
    m.plane[2] = m.plane[1] + c->n * sizeof(unsigned);
    m.sums = (unsigned long long *)(call->db + call->extra_off) + i;
    m.nblk = cvh_cc_blocks(c->n);
  }
  return CVH_OK;
}

int components(cvh_context *const *ctxs, int n, int conn, int invert, int32_t *const *d_labels, int *counts, cvh_component *table, int cap,
               void *stream, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  rc = conn_check(ctxs, n, conn, what);
  if (rc != CVH_OK) return rc;
  if (table && cap < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: cap must not be negative, got %d", what, cap);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  bool any_labels = false;
  for (int i = 0; d_labels && i < n; ++i) {
    if (!d_labels[i]) continue;   // (no label plane for this member)
    rc = pointer_check(ctxs, n, i, d_labels[i], what);
    if (rc != CVH_OK) return rc;
    if ((uintptr_t)d_labels[i] % sizeof(int32_t))
      return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: %p is not aligned to 4 bytes", what, i, (const void *)d_labels[i]);
    any_labels = true;
  }
  rc = members_ready(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  MemberCall call;
  rc = fill_members(&call, ctxs, n, (void *const *)d_labels, what);
  if (rc != CVH_OK) return rc;
  const unsigned long long *words = (const unsigned long long *)(call.hb + call.extra_off);
  rc = call.run(stream, any_labels, true, [&]() -> int {   // the host wait of the call: the counts
    HIPCHK(lead, cvh_launch_cc_label(call.dtab(), n, call.grid, conn, invert, any_labels, lead->stream));
    HIPCHK(lead, hipMemcpyAsync((void *)words, call.db + call.extra_off, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, lead->stream));
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; counts && i < n; ++i) counts[i] = (int)words[i];
  const size_t K = (size_t)words[0];
  const size_t rows = std::min<size_t>(K, table ? (size_t)cap : 0);
  if (!rows) return CVH_OK;
  // the table (single-context form): K is known now, so the rows have their place; two more launches on the workspace, then the SECOND wait
  if (lead->cc_table_rows < K) {
    if (lead->d_cc_table) { HIPCHK(lead, hipFree(lead->d_cc_table)); lead->d_cc_table = nullptr; lead->cc_table_rows = 0; }
    const size_t want = K + K / 4;
    HIPCHK(lead, hipMalloc(&lead->d_cc_table, want * sizeof(cvh_component)));
    lead->cc_table_rows = want;
  }
  call.tab[0].dst = lead->d_cc_table;   // (the label plane is written: these launches fill the rows)
  HIPCHK(lead, hipMemcpyAsync(call.db, call.hb, sizeof(CvhIoMember), hipMemcpyHostToDevice, lead->stream));
  HIPCHK(lead, cvh_launch_cc_table(call.dtab(), 1, call.grid, lead->stream));
  HIPCHK(lead, hipMemcpyAsync(table, lead->d_cc_table, rows * sizeof(cvh_component), hipMemcpyDeviceToHost, lead->stream));
  HIPCHK(lead, hipEventRecord(lead->ev_io_out, lead->stream));   // (the last read of the pinned block)
  HIPCHK(lead, hipStreamSynchronize(lead->stream));
  return CVH_OK;
}

int clean_args(cvh_context *const *ctxs, int n, int conn, long min_area, long fill_holes, int keep_largest, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  rc = conn_check(ctxs, n, conn, what);
  if (rc != CVH_OK) return rc;
  if (min_area < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: min_area must not be negative, got %ld", what, min_area);
  if (fill_holes < -1) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: fill_holes must be -1 (any size) or an area >= 0, got %ld", what, fill_holes);
  if (keep_largest != 0 && keep_largest != 1) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: keep_largest must be 0 or 1, got %d", what, keep_largest);
  return CVH_OK;
}

int clean(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, int conn, int invert, long min_area, long fill_holes, int keep_largest,
          void *stream, const char *what)
{
  int rc = clean_args(ctxs, n, conn, min_area, fill_holes, keep_largest, what);
  if (rc != CVH_OK) return rc;
  const bool drop = min_area > 1;   // (every component has a pixel)
  if (!drop && !fill_holes && !keep_largest) return mask_out(ctxs, n, d_masks, invert, stream, what);   // the existing mask kernel alone
  if (!d_masks) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of device pointers is NULL", what);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; i < n; ++i) { rc = pointer_check(ctxs, n, i, d_masks[i], what); if (rc != CVH_OK) return rc; }
  rc = members_ready(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  MemberCall call;
  rc = fill_members(&call, ctxs, n, (void *const *)d_masks, what);
  if (rc != CVH_OK) return rc;
  return call.run(stream, true, false, [&]() -> int {
    if (!drop) HIPCHK(lead, cvh_launch_io_mask(call.dtab(), n, call.grid, invert, lead->stream));   // step 1 is off: the plain mask
    const unsigned a = (unsigned)std::min<long>(min_area, 0x7fffffffl);
    HIPCHK(lead, cvh_launch_cc_clean(call.dtab(), n, call.grid, conn, invert, a, fill_holes, keep_largest, lead->stream));
    return CVH_OK;
  });
}

}  // namespace

// measure_run.hip takes the same argument checks, the same readiness and the same member table as the calls here
int cc_clean_args(cvh_context *const *ctxs, int n, int conn, long min_area, long fill_holes, int keep_largest, const char *what)
{
  return clean_args(ctxs, n, conn, min_area, fill_holes, keep_largest, what);
}
int cc_members_ready(cvh_context *const *ctxs, int n, const char *what) { return members_ready(ctxs, n, what); }
int cc_fill_members(MemberCall *call, cvh_context *const *ctxs, int n, void *const *dst, const char *what, bool two_tables, size_t more)
{
  return fill_members(call, ctxs, n, dst, what, two_tables, more);
}

extern "C" int cvh_components_batch(cvh_context *const *ctxs, int n, int conn, int invert, int32_t *const *d_labels, int *counts, void *stream)
{
  static const char what[] = "cvh_components_batch";
  return guarded(ctxs, n, what, [&]() { return components(ctxs, n, conn, invert, d_labels, counts, nullptr, 0, stream, what); });
}

extern "C" int cvh_components(cvh_context *c, int conn, int invert, int32_t *d_labels, cvh_component *table, int cap, int *count, void *stream)
{
  return guarded_one(c, "cvh_components", [&](const char *what) { return components(&c, 1, conn, invert, &d_labels, count, table, cap, stream, what); });
}

extern "C" int cvh_get_mask_clean_device_batch(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, int conn, int invert, long min_area,
                                               long fill_holes, int keep_largest, void *stream)
{
  static const char what[] = "cvh_get_mask_clean_device_batch";
  return guarded(ctxs, n, what, [&]() { return clean(ctxs, n, d_masks, conn, invert, min_area, fill_holes, keep_largest, stream, what); });
}

extern "C" int cvh_get_mask_clean_device(cvh_context *c, uint8_t *d_mask, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                         void *stream)
{
  return guarded_one(c, "cvh_get_mask_clean_device", [&](const char *what) { return clean(&c, 1, &d_mask, conn, invert, min_area, fill_holes, keep_largest, stream, what); });
}

extern "C" int cvh_get_mask_clean(cvh_context *c, uint8_t *mask, int conn, int invert, long min_area, long fill_holes, int keep_largest)
{
  return guarded_one(c, "cvh_get_mask_clean", [&](const char *what) {
    if (!mask) return fail(c, CVH_ERR_ARG, "%s: mask is NULL", what);
    int rc = clean_args(&c, 1, conn, min_area, fill_holes, keep_largest, what);
    if (rc != CVH_OK) return rc;
    if (!c->have_u) return fail(c, CVH_ERR_STATE, "%s: no level set", what);
    return mask_to_host(c, mask, [&]() { return clean(&c, 1, &c->d_mask, conn, invert, min_area, fill_holes, keep_largest, c->stream, what); });
  });
}
