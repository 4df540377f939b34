// components_run.hip — host side of cvh_components* and cvh_get_mask_clean* (include/chanvese_hip.h, "Connected components"): read-only
// operations on the level sets of n contexts, each ONE MemberCall (cvh_host.h, io_run.hip: member table, stream joins, event ordering).
// The single-context calls are batches of one member (guarded_one); what the members must hold is asked of csv_batch.hip's predicates.
// MaskSource (cvh_host.h) is defined here: the one path by which these calls, and those of measure_run.hip, overlap_run.hip,
// contour_run.hip and morph_run.hip, come by the raw or cleaned mask of every member -- argument checks, readiness, the first member
// table, the mask launches.  Nothing here touches a context's level set, run state, sums or options.
#include "cvh_host.h"

int MaskSource::check(cvh_context *const *ctxs, int n, const char *what) const
{
  const int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  if (conn != 4 && conn != 8) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: conn must be 4 or 8, got %d", what, conn);
  if (min_area < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: min_area must not be negative, got %ld", what, min_area);
  if (fill_holes < -1) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: fill_holes must be -1 (any size) or an area >= 0, got %ld", what, fill_holes);
  if (keep_largest != 0 && keep_largest != 1) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: keep_largest must be 0 or 1, got %d", what, keep_largest);
  return CVH_OK;
}

int MaskSource::ready(cvh_context *const *ctxs, int n, const char *what, bool need_cc) const
{
  if (!need_cc && !cleaned()) {   // the plain mask kernel alone reads the level sets
    int rc = members_have_levelsets(ctxs, n, what);
    if (rc == CVH_OK) rc = settle_all(ctxs, n, what);
    return rc != CVH_OK ? rc : members_mirrors_fresh(ctxs, n, what);
  }
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

void MaskSource::fill(MemberCall *call, int i, void *dst, unsigned long long *sums, bool need_cc) const
{
  const cvh_context *c = call->ctxs[i];
  CvhIoMember &m = call->tab[i];
  m.src = c->d_u[current_buffer(c)];
  m.dst = dst;
  if (need_cc || cleaned()) {
    m.plane[0] = (uint8_t *)c->d_cc;
    m.plane[1] = m.plane[0] + c->n * sizeof(unsigned);
    m.plane[2] = m.plane[1] + c->n * sizeof(unsigned);
  }
  m.sums = sums;
  m.nblk = cvh_cc_blocks(c->n);
}

int MaskSource::launch(const MemberCall &call, bool raw_too) const
{
  cvh_context *lead = call.lead;
  if (!cleaned() && !raw_too) return CVH_OK;
  if (!drop()) HIPCHK(lead, cvh_launch_io_mask(call.dtab(), call.n, call.grid, invert, lead->stream));   // step 1 is off: the plain mask
  if (!cleaned()) return CVH_OK;
  const unsigned a = (unsigned)std::min<long>(min_area, 0x7fffffffl);
  HIPCHK(lead, cvh_launch_cc_clean(call.dtab(), call.n, call.grid, conn, invert, a, fill_holes, keep_largest, lead->stream));
  return CVH_OK;
}

namespace {

// staging: [member table][one word per member, zero at extra_off].  dst[i] is member i's output (may be null, and so may dst)
int begin_and_fill(MemberCall *call, const MaskSource &src, cvh_context *const *ctxs, int n, void *const *dst, const char *what)
{
  const int rc = call->begin(ctxs, n, what, (size_t)n * sizeof(unsigned long long));
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) src.fill(call, i, dst ? dst[i] : nullptr, (unsigned long long *)(call->db + call->extra_off) + i, true);
  return CVH_OK;
}

int components(cvh_context *const *ctxs, int n, int conn, int invert, int32_t *const *d_labels, int *counts, cvh_component *table, int cap,
               void *stream, const char *what)
{
  const MaskSource src = {conn, invert};   // the raw mask: the labelling launch reads the level sets itself
  int rc = src.check(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (table && cap < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: cap must not be negative, got %d", what, cap);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  bool any_labels = false;
  for (int i = 0; d_labels && i < n; ++i) {
    if (!d_labels[i]) continue;   // (no label plane for this member)
    rc = element_pointer_check(ctxs, n, i, d_labels[i], sizeof(int32_t), what);
    if (rc != CVH_OK) return rc;
    any_labels = true;
  }
  rc = src.ready(ctxs, n, what, true);
  if (rc != CVH_OK) return rc;
  MemberCall call;
  rc = begin_and_fill(&call, src, ctxs, n, (void *const *)d_labels, what);
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
  rc = grow_table_to(lead, &lead->cc_table, K, K + K / 4, (K + K / 4) * sizeof(cvh_component));
  if (rc != CVH_OK) return rc;
  call.tab[0].dst = lead->cc_table.d;   // (the label plane is written: these launches fill the rows)
  rc = call.upload_again(call.tab);
  if (rc != CVH_OK) return rc;
  HIPCHK(lead, cvh_launch_cc_table(call.dtab(), 1, call.grid, lead->stream));
  HIPCHK(lead, hipMemcpyAsync(table, lead->cc_table.d, rows * sizeof(cvh_component), hipMemcpyDeviceToHost, lead->stream));
  return call.wait_again(stream, false);
}

int clean(cvh_context *const *ctxs, int n, uint8_t *const *d_masks, const MaskSource &src, void *stream, const char *what)
{
  int rc = src.check(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (!src.cleaned()) return mask_out(ctxs, n, d_masks, src.invert, stream, what);   // the existing mask kernel alone
  if (!d_masks) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of device pointers is NULL", what);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; i < n; ++i) { rc = pointer_check(ctxs, n, i, d_masks[i], what); if (rc != CVH_OK) return rc; }
  rc = src.ready(ctxs, n, what, true);
  if (rc != CVH_OK) return rc;
  MemberCall call;
  rc = begin_and_fill(&call, src, ctxs, n, (void *const *)d_masks, what);
  if (rc != CVH_OK) return rc;
  return call.run(stream, true, false, [&]() { return src.launch(call, false); });
}

}  // namespace

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
  return guarded(ctxs, n, what, [&]() { return clean(ctxs, n, d_masks, {conn, invert, min_area, fill_holes, keep_largest}, stream, what); });
}

extern "C" int cvh_get_mask_clean_device(cvh_context *c, uint8_t *d_mask, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                         void *stream)
{
  return guarded_one(c, "cvh_get_mask_clean_device", [&](const char *what) {
    return clean(&c, 1, &d_mask, {conn, invert, min_area, fill_holes, keep_largest}, stream, what);
  });
}

extern "C" int cvh_get_mask_clean(cvh_context *c, uint8_t *mask, int conn, int invert, long min_area, long fill_holes, int keep_largest)
{
  return guarded_one(c, "cvh_get_mask_clean", [&](const char *what) {
    const MaskSource src = {conn, invert, min_area, fill_holes, keep_largest};
    if (!mask) return fail(c, CVH_ERR_ARG, "%s: mask is NULL", what);
    const int rc = src.check(&c, 1, what);
    if (rc != CVH_OK) return rc;
    if (!c->have_u) return fail(c, CVH_ERR_STATE, "%s: no level set", what);
    return mask_to_host(c, mask, [&]() { return clean(&c, 1, &c->d_mask, src, c->stream, what); });
  });
}
