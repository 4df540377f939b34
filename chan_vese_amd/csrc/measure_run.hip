// measure_run.hip — host side of cvh_measure* (include/chanvese_hip.h, "Component measures"): the components of the masks of n contexts,
// raw or cleaned, measured on the device -- ONE MemberCall (cvh_host.h, io_run.hip) with two member tables: the mask source's
// (MaskSource, components_run.hip; the workspace in plane[]) for the cleaning and numbering launches, and a second one (the image in
// plane[]) for measure_kernels.hip.  The single-context form is a batch of one.  The calls only read: nothing of a member's level set, run state,
// sums, options or planes is assigned here.  cvh_region_shape_of, the host arithmetic on a row, lives here too.
#include "cvh_host.h"

namespace {

int measure(cvh_context *const *ctxs, int n, const MaskSource &src, cvh_region *const *tables, const int *caps, int *counts, void *stream,
            const char *what)
{
  int rc = src.check(ctxs, n, what);
  if (rc == CVH_OK) rc = members_caps_fit(ctxs, n, what, (const void *const *)tables, caps, "cap", "tables without caps");
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i)   // (with h w < 2^31 this keeps every sum below 2^63)
    if (ctxs[i]->h > 65535 || ctxs[i]->w > 65535)
      return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: %d x %d is too large, h and w must stay below 65536", what, i, ctxs[i]->h, ctxs[i]->w);
  rc = members_below(ctxs, n, what, 31);
  if (rc == CVH_OK) rc = members_have_images(ctxs, n, what);
  if (rc == CVH_OK) rc = src.ready(ctxs, n, what, true);
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  const bool cleaned = src.cleaned();
  std::vector<void *> masks((size_t)n, nullptr);
  for (int i = 0; cleaned && i < n; ++i) {   // the cleaned mask goes to the context's own mask buffer (cvh_get_mask's) and is labelled there
    cvh_context *c = ctxs[i];
    if (!c->d_mask) HIPCHK(lead, hipMalloc((void **)&c->d_mask, c->n));
    masks[(size_t)i] = c->d_mask;
  }
  // staging: [the mask launches' table][the measure launches' table][one word per member, zero]
  MemberCall call;
  rc = call.begin(ctxs, n, what, (size_t)n * sizeof(unsigned long long), 0, true);
  if (rc != CVH_OK) return rc;
  bool any_c1 = false, any_c3 = false;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    src.fill(&call, i, masks[(size_t)i], (unsigned long long *)(call.db + call.extra_off) + i, true);
    CvhIoMember &m = call.tab2[i];
    m.src = c->d_cc;
    for (int k = 0; k < c->C; ++k) m.plane[k] = c->d_img[k];
    m.nblk = cvh_measure_blocks(c->n);
    (c->C == 1 ? any_c1 : any_c3) = true;
  }
  const unsigned long long *words = (const unsigned long long *)(call.hb + call.extra_off);
  rc = call.run(stream, false, true, [&]() -> int {   // the first host wait of the call: the counts
    const int rc_mask = src.launch(call, false);   // (keep_largest has used the members' words for its bids: the scan of the numbering stores K over them)
    if (rc_mask != CVH_OK) return rc_mask;
    HIPCHK(lead, cvh_launch_cc_number(call.dtab(), n, call.grid, cleaned ? 1 : 0, src.conn, src.invert, lead->stream));
    HIPCHK(lead, hipMemcpyAsync((void *)words, call.db + call.extra_off, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, lead->stream));
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  for (int i = 0; counts && i < n; ++i) counts[i] = (int)words[i];
  // the rows: K is known now, so they have their place; the measure launches on the second table, then the SECOND wait
  bool any_rows = false;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    const size_t rows = std::min<size_t>((size_t)words[i], tables && tables[i] ? (size_t)caps[i] : 0);
    if (!rows) continue;
    rc = grow_table_to(lead, &c->regions, rows, rows + rows / 4, (rows + rows / 4) * sizeof(cvh_region));
    if (rc != CVH_OK) return rc;
    call.tab2[i].dst = c->regions.d;
    call.tab2[i].h2 = (int)rows;
    any_rows = true;
  }
  if (!any_rows) return CVH_OK;
  rc = call.upload_again(call.tab2);
  if (rc != CVH_OK) return rc;
  HIPCHK(lead, cvh_launch_measure(call.dtab2(), n, call.grid2, any_c1, any_c3, lead->stream));
  for (int i = 0; i < n; ++i)
    if (call.tab2[i].h2)
      HIPCHK(lead, hipMemcpyAsync(tables[i], ctxs[i]->regions.d, (size_t)call.tab2[i].h2 * sizeof(cvh_region), hipMemcpyDeviceToHost, lead->stream));
  return call.wait_again(stream, false);
}

// v as a double, rounded to nearest even ONCE (what Python's float(int) gives)
double to_double(unsigned __int128 v)
{
  const uint64_t hi = (uint64_t)(v >> 64), lo = (uint64_t)v;
  if (!hi) return (double)lo;
  const int shift = 64 - __builtin_clzll(hi);   // 1 .. 64: the top 64 bits of v are v >> shift
  uint64_t top = (uint64_t)(v >> shift);
  if (v & ((((unsigned __int128)1) << shift) - 1)) top |= 1;   // sticky: eleven bits below the rounding position of a double
  return ldexp((double)top, shift);
}

// (a b - c d) / A^2 with the numerator an exact 128-bit integer
double central(uint64_t a, uint64_t b, uint64_t c, uint64_t d, double A2)
{
  const unsigned __int128 x = (unsigned __int128)a * b, y = (unsigned __int128)c * d;
  return x >= y ? to_double(x - y) / A2 : -to_double(y - x) / A2;
}

}  // namespace

extern "C" int cvh_measure_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                 cvh_region *const *tables, const int *caps, int *counts, void *stream)
{
  static const char what[] = "cvh_measure_batch";
  return guarded(ctxs, n, what, [&]() { return measure(ctxs, n, {conn, invert, min_area, fill_holes, keep_largest}, tables, caps, counts, stream, what); });
}

extern "C" int cvh_measure(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, cvh_region *table, int cap,
                           int *count, void *stream)
{
  return guarded_one(c, "cvh_measure", [&](const char *what) {
    if (table && cap < 0) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: cap must not be negative, got %d", what, cap);
    return measure(&c, 1, {conn, invert, min_area, fill_holes, keep_largest}, &table, &cap, count, stream, what);
  });
}

extern "C" int cvh_region_shape_of(const cvh_region *r, int channels, cvh_region_shape *out)
{
  if (!r || !out || (channels != 1 && channels != 3) || r->area == 0) return CVH_ERR_ARG;
  memset(out, 0, sizeof(*out));
  const uint64_t A = r->area;
  const double a = (double)A, A2 = a * a;
  out->cx = (double)r->sx / a;
  out->cy = (double)r->sy / a;
  out->mu20 = central(A, r->sxx, r->sx, r->sx, A2);
  out->mu02 = central(A, r->syy, r->sy, r->sy, A2);
  out->mu11 = central(A, r->sxy, r->sx, r->sy, A2);
  for (int k = 0; k < channels; ++k) {
    out->mean[k] = (double)r->s1[k] / a;
    out->var[k] = central(A, r->s2[k], r->s1[k], r->s1[k], A2);
  }
  const double half = (out->mu20 - out->mu02) / 2, mid = (out->mu20 + out->mu02) / 2;
  const double root = sqrt(half * half + out->mu11 * out->mu11);
  const double l1 = mid + root, l2 = mid - root;
  out->theta = 0.5 * atan2(2 * out->mu11, out->mu20 - out->mu02);
  out->major = 4 * sqrt(l1);
  out->minor = l2 < 0 ? 0.0 : 4 * sqrt(l2);
  return CVH_OK;
}
