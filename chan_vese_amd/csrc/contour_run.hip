// contour_run.hip — host side of cvh_contours* and cvh_contours_subpixel* (include/chanvese_hip.h, "Contours", "Subpixel contours"): the boundaries of the masks of n contexts, raw or
// cleaned, as ordered closed loops -- ONE MemberCall (cvh_host.h, io_run.hip) with two member tables: the mask source's (MaskSource,
// components_run.hip: the level set in src, the mask bytes in dst, the components workspace in plane[]) for the mask or cleaning
// launches, and a second one for contour_kernels.hip.  The single-context forms are batches of one.  The calls only read: nothing of a member's level set, run state,
// sums, options or planes is assigned here.  Two host waits: the edge counts (they size the per-edge workspace, the sections of the
// edge launches and the rounds of the doubling), then the loop and point counts with the rows.  The subpixel calls are the same path with
// another kind of point (Outputs::subpixel): the trace runs unsimplified and its last launch gathers the crossings from the level sets.
#include "cvh_host.h"

namespace {

struct Outputs {
  cvh_contour_loop *const *loops;   // host tables (may be null, and so may an entry)
  const long *loop_caps;
  void *const *points;              // device pointers, or with on_host host pointers (may be null, and so may an entry)
  const long *point_caps;
  long *nloops, *npoints;           // arrays of n, or null
  bool on_host;
  bool subpixel;                    // a point is the zero level's crossing of its edge, two doubles; else the edge's tail vertex, two int32
  size_t point_bytes() const { return subpixel ? 2 * sizeof(double) : 2 * sizeof(int32_t); }
};

int contours(cvh_context *const *ctxs, int n, const MaskSource &src, int simplify, const Outputs &out, void *stream, const char *what)
{
  int rc = src.check(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (out.subpixel) simplify = 0;   // (one point per edge)
  else if (simplify != 0 && simplify != 1) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: simplify must be 0 or 1, got %d", what, simplify);
  for (int i = 0; i < n; ++i) {   // (member by member: a member's points before the next member's loops)
    rc = members_caps_fit(ctxs, n, what, (const void *const *)out.loops, out.loop_caps, "loop_cap", "loop tables without loop_caps", i);
    if (rc == CVH_OK) rc = members_caps_fit(ctxs, n, what, (const void *const *)out.points, out.point_caps, "point_cap", "point arrays without point_caps", i);
    if (rc != CVH_OK) return rc;
  }
  rc = members_below(ctxs, n, what, 30);   // (an edge id, 4 p + k, is 32 bits)
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; !out.on_host && out.points && i < n; ++i) {
    if (!out.points[i]) continue;
    rc = element_pointer_check(ctxs, n, i, out.points[i], out.subpixel ? sizeof(double) : sizeof(int32_t), what);
    if (rc != CVH_OK) return rc;
  }
  rc = src.ready(ctxs, n, what, false);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    rc = ensure_workspace(c, &c->d_contour, cvh_contour_pixel_bytes(c->n), "contour", false);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, c->err);
  }
  // staging: [the mask launches' table][the contour launches' table][one word per member for the cleaning, then {E, loops, points, 0}]
  MemberCall call;
  rc = call.begin(ctxs, n, what, (size_t)n * 5 * sizeof(unsigned long long), 0, true);
  if (rc != CVH_OK) return rc;
  unsigned long long *const words = (unsigned long long *)(call.hb + call.extra_off) + n;
  unsigned long long *const d_words = (unsigned long long *)(call.db + call.extra_off) + n;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    uint8_t *const base = (uint8_t *)c->d_contour;
    src.fill(&call, i, base, (unsigned long long *)(call.db + call.extra_off) + i, false);
    CvhIoMember &t = call.tab2[i];
    t.src = base;
    t.plane[0] = base + cvh_contour_bits_offset(c->n);
    t.plane[1] = base + cvh_contour_prefix_offset(c->n);
    t.plane[2] = base + cvh_contour_counts_offset(c->n);
    t.sums = d_words + 4 * (size_t)i;
    t.nblk = cvh_cc_blocks(c->n);
  }
  rc = call.run(stream, false, true, [&]() -> int {   // the first host wait of the call: the edge counts
    const int rc_mask = src.launch(call, true);   // (a raw mask too: the count launch reads the mask bytes)
    if (rc_mask != CVH_OK) return rc_mask;
    HIPCHK(lead, cvh_launch_contours_count(call.dtab2(), n, call.grid2, lead->stream));
    HIPCHK(lead, hipMemcpyAsync(words, d_words, (size_t)n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, lead->stream));
    return CVH_OK;
  });
  if (rc != CVH_OK) return rc;
  size_t max_edges = 0;
  for (int i = 0; i < n; ++i) max_edges = std::max<size_t>(max_edges, (size_t)words[4 * i]);
  if (!max_edges) {   // empty masks: no loops, no error
    for (int i = 0; i < n; ++i) { if (out.nloops) out.nloops[i] = 0; if (out.npoints) out.npoints[i] = 0; }
    return CVH_OK;
  }
  // E is known: the per-edge workspaces have their size, the edge launches their sections and the doubling its rounds
  int rounds = 0;
  while (((size_t)1 << rounds) < max_edges) ++rounds;
  bool any_points = false;
  std::vector<size_t> row_room((size_t)n, 0), point_room((size_t)n, 0);   // what can come back at most: a loop has >= 4 edges, a point an edge
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    const size_t E = (size_t)words[4 * i];
    CvhIoMember &t = call.tab2[i];
    t.nblk = cvh_contour_edge_blocks(E, c->n);
    if (!E) continue;
    rc = grow_table_to(lead, &c->contour_edges, E, E + E / 4, cvh_contour_edge_bytes(E + E / 4));
    if (rc != CVH_OK) return rc;
    t.dst = c->contour_edges.d;
    t.src_stride = c->contour_edges.count;
    if (out.loops && out.loops[i]) row_room[(size_t)i] = std::min<size_t>((size_t)out.loop_caps[i], E / 4);
    if (!out.points || !out.points[i]) continue;
    const unsigned long long cap = (unsigned long long)out.point_caps[i];
    point_room[(size_t)i] = (size_t)std::min<unsigned long long>(cap, E);
    if (out.on_host) {
      if (!point_room[(size_t)i]) continue;
      const size_t room = point_room[(size_t)i], units = out.point_bytes() / 8;   // (the table counts 8-byte units: both kinds of point share it)
      rc = grow_table_to(lead, &c->contour_points, room * units, (room + room / 4) * units, (room + room / 4) * out.point_bytes());
      if (rc != CVH_OK) return rc;
      t.src2 = c->contour_points.d;
    } else {
      t.src2 = out.points[i];
    }
    t.h2 = (int)(unsigned)cap; t.w2 = (int)(unsigned)(cap >> 32);
    any_points = true;
  }
  call.grid2 = lay_out(call.tab2, n);
  std::vector<std::vector<cvh_contour_loop>> rows((size_t)n);
  std::vector<std::vector<uint8_t>> pts((size_t)n);
  rc = call.upload_again(call.tab2);
  if (rc != CVH_OK) return rc;
  HIPCHK(lead, cvh_launch_contours_trace(call.dtab2(), n, call.grid2, src.conn, simplify, rounds, any_points, out.subpixel ? call.dtab() : nullptr,
                                         src.invert, lead->stream));
  HIPCHK(lead, hipMemcpyAsync(words, d_words, (size_t)n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, lead->stream));
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    if (row_room[(size_t)i]) {
      rows[(size_t)i].resize(row_room[(size_t)i]);
      HIPCHK(lead, hipMemcpyAsync(rows[(size_t)i].data(), (const uint8_t *)c->contour_edges.d + cvh_contour_rows_offset(c->contour_edges.count),
                                  row_room[(size_t)i] * sizeof(cvh_contour_loop), hipMemcpyDeviceToHost, lead->stream));
    }
    if (out.on_host && point_room[(size_t)i]) {
      pts[(size_t)i].resize(point_room[(size_t)i] * out.point_bytes());
      HIPCHK(lead, hipMemcpyAsync(pts[(size_t)i].data(), c->contour_points.d, point_room[(size_t)i] * out.point_bytes(), hipMemcpyDeviceToHost, lead->stream));
    }
  }
  rc = call.wait_again(stream, !out.on_host && any_points);   // the SECOND host wait: counts and rows (the caller's stream waits for its points)
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const size_t L = (size_t)words[4 * i + 1], P = (size_t)words[4 * i + 2];
    if (out.nloops) out.nloops[i] = (long)L;
    if (out.npoints) out.npoints[i] = (long)P;
    if (row_room[(size_t)i]) memcpy(out.loops[i], rows[(size_t)i].data(), std::min(L, row_room[(size_t)i]) * sizeof(cvh_contour_loop));
    if (out.on_host && point_room[(size_t)i]) memcpy(out.points[i], pts[(size_t)i].data(), std::min(P, point_room[(size_t)i]) * out.point_bytes());
  }
  return CVH_OK;
}

int single(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, int simplify, cvh_contour_loop *loops,
           long loop_cap, void *points, long point_cap, long *nloops, long *npoints, void *stream, bool on_host, bool subpixel, const char *what)
{
  if (loop_cap < 0) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: loop_cap must not be negative, got %ld", what, loop_cap);
  if (point_cap < 0) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: point_cap must not be negative, got %ld", what, point_cap);
  const Outputs out = {&loops, &loop_cap, &points, &point_cap, nloops, npoints, on_host, subpixel};
  return contours(&c, 1, {conn, invert, min_area, fill_holes, keep_largest}, simplify, out, stream, what);
}

}  // namespace

extern "C" int cvh_contours_device_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                         int simplify, cvh_contour_loop *const *loops, const long *loop_caps, int32_t *const *d_points,
                                         const long *point_caps, long *nloops, long *npoints, void *stream)
{
  static const char what[] = "cvh_contours_device_batch";
  const Outputs out = {loops, loop_caps, (void *const *)d_points, point_caps, nloops, npoints, false, false};
  return guarded(ctxs, n, what, [&]() { return contours(ctxs, n, {conn, invert, min_area, fill_holes, keep_largest}, simplify, out, stream, what); });
}

extern "C" int cvh_contours_device(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, int simplify,
                                   cvh_contour_loop *loops, long loop_cap, int32_t *d_points, long point_cap, long *nloops, long *npoints,
                                   void *stream)
{
  return guarded_one(c, "cvh_contours_device", [&](const char *what) {
    return single(c, conn, invert, min_area, fill_holes, keep_largest, simplify, loops, loop_cap, d_points, point_cap, nloops, npoints, stream, false, false, what);
  });
}

extern "C" int cvh_contours(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, int simplify,
                            cvh_contour_loop *loops, long loop_cap, int32_t *points, long point_cap, long *nloops, long *npoints)
{
  return guarded_one(c, "cvh_contours", [&](const char *what) {
    return single(c, conn, invert, min_area, fill_holes, keep_largest, simplify, loops, loop_cap, points, point_cap, nloops, npoints, c->stream, true, false, what);
  });
}

extern "C" int cvh_contours_subpixel_device_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                                  cvh_contour_loop *const *loops, const long *loop_caps, double *const *d_points,
                                                  const long *point_caps, long *nloops, long *npoints, void *stream)
{
  static const char what[] = "cvh_contours_subpixel_device_batch";
  const Outputs out = {loops, loop_caps, (void *const *)d_points, point_caps, nloops, npoints, false, true};
  return guarded(ctxs, n, what, [&]() { return contours(ctxs, n, {conn, invert, min_area, fill_holes, keep_largest}, 0, out, stream, what); });
}

extern "C" int cvh_contours_subpixel_device(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                            cvh_contour_loop *loops, long loop_cap, double *d_points, long point_cap, long *nloops, long *npoints,
                                            void *stream)
{
  return guarded_one(c, "cvh_contours_subpixel_device", [&](const char *what) {
    return single(c, conn, invert, min_area, fill_holes, keep_largest, 0, loops, loop_cap, d_points, point_cap, nloops, npoints, stream, false, true, what);
  });
}

extern "C" int cvh_contours_subpixel(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                     cvh_contour_loop *loops, long loop_cap, double *points, long point_cap, long *nloops, long *npoints)
{
  return guarded_one(c, "cvh_contours_subpixel", [&](const char *what) {
    return single(c, conn, invert, min_area, fill_holes, keep_largest, 0, loops, loop_cap, points, point_cap, nloops, npoints, c->stream, true, true, what);
  });
}

// area and length of the polygon of one loop's n subpixel points: sequential FP64 sums in index order (host only; no context, no message)
extern "C" int cvh_contour_subpixel_measure(const double *points, long n, double *area, double *length)
{
  if (n < 0 || !points || !area || !length) return CVH_ERR_ARG;
  double cross = 0.0, len = 0.0;
  for (long i = 0; i < n; ++i) {
    const long j = i + 1 < n ? i + 1 : 0;
    const double x0 = points[2 * i], y0 = points[2 * i + 1], x1 = points[2 * j], y1 = points[2 * j + 1];
    const double dx = x1 - x0, dy = y1 - y0;
    cross += x0 * y1 - x1 * y0;
    len += sqrt(dx * dx + dy * dy);
  }
  *area = 0.5 * cross;
  *length = len;
  return CVH_OK;
}
