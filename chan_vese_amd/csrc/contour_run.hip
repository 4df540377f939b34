// contour_run.hip — host side of cvh_contours* (include/chanvese_hip.h, "Contours"): the boundaries of the masks of n contexts, raw or
// cleaned, as ordered closed loops -- ONE MemberCall (cvh_host.h, io_run.hip) with two member tables: the components calls' layout (the
// level set in src, the mask bytes in dst, the components workspace in plane[]) for the mask or cleaning launches, and a second one for
// contour_kernels.hip.  The single-context forms are batches of one.  The calls only read: nothing of a member's level set, run state,
// sums, options or planes is assigned here.  Two host waits: the edge counts (they size the per-edge workspace, the sections of the
// edge launches and the rounds of the doubling), then the loop and point counts with the rows.
#include "cvh_host.h"

namespace {

struct Outputs {
  cvh_contour_loop *const *loops;   // host tables (may be null, and so may an entry)
  const long *loop_caps;
  int32_t *const *points;           // device pointers, or with on_host host pointers (may be null, and so may an entry)
  const long *point_caps;
  long *nloops, *npoints;           // arrays of n, or null
  bool on_host;
};

int grow(cvh_context *lead, void **slot, size_t *have, size_t want, size_t unit)
{
  if (*have >= want) return CVH_OK;
  if (*slot) { HIPCHK(lead, hipFree(*slot)); *slot = nullptr; *have = 0; }
  const size_t cap = want + want / 4;
  HIPCHK(lead, hipMalloc(slot, unit ? cap * unit : cvh_contour_edge_bytes(cap)));
  *have = cap;
  return CVH_OK;
}

int contours(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest, int simplify,
             const Outputs &out, void *stream, const char *what)
{
  int rc = cc_clean_args(ctxs, n, conn, min_area, fill_holes, keep_largest, what);
  if (rc != CVH_OK) return rc;
  if (simplify != 0 && simplify != 1) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: simplify must be 0 or 1, got %d", what, simplify);
  for (int i = 0; i < n; ++i) {
    if (out.loops && out.loops[i]) {
      if (!out.loop_caps) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: loop tables without loop_caps", what);
      if (out.loop_caps[i] < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: loop_cap must not be negative, got %ld", what, i, out.loop_caps[i]);
    }
    if (out.points && out.points[i]) {
      if (!out.point_caps) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: point arrays without point_caps", what);
      if (out.point_caps[i] < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: point_cap must not be negative, got %ld", what, i, out.point_caps[i]);
    }
  }
  rc = members_below(ctxs, n, what, 30);   // (an edge id, 4 p + k, is 32 bits)
  if (rc != CVH_OK) return rc;
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  for (int i = 0; !out.on_host && out.points && i < n; ++i) {
    if (!out.points[i]) continue;
    rc = pointer_check(ctxs, n, i, out.points[i], what);
    if (rc != CVH_OK) return rc;
    if ((uintptr_t)out.points[i] % sizeof(int32_t))
      return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: %p is not aligned to 4 bytes", what, i, (const void *)out.points[i]);
  }
  const bool drop = min_area > 1, cleaned = drop || fill_holes || keep_largest;
  if (cleaned) rc = cc_members_ready(ctxs, n, what);
  else {
    rc = members_have_levelsets(ctxs, n, what);
    if (rc == CVH_OK) rc = settle_all(ctxs, n, what);
    if (rc == CVH_OK) rc = members_mirrors_fresh(ctxs, n, what);
  }
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
    CvhIoMember &m = call.tab[i];
    m.src = c->d_u[current_buffer(c)];
    m.dst = base;
    if (cleaned) {
      m.plane[0] = (uint8_t *)c->d_cc;
      m.plane[1] = m.plane[0] + c->n * sizeof(unsigned);
      m.plane[2] = m.plane[1] + c->n * sizeof(unsigned);
    }
    m.sums = (unsigned long long *)(call.db + call.extra_off) + i;
    m.nblk = cvh_cc_blocks(c->n);
    CvhIoMember &t = call.tab2[i];
    t.src = base;
    t.plane[0] = base + cvh_contour_bits_offset(c->n);
    t.plane[1] = base + cvh_contour_prefix_offset(c->n);
    t.plane[2] = base + cvh_contour_counts_offset(c->n);
    t.sums = d_words + 4 * (size_t)i;
    t.nblk = cvh_cc_blocks(c->n);
  }
  rc = call.run(stream, false, true, [&]() -> int {   // the first host wait of the call: the edge counts
    if (!drop) HIPCHK(lead, cvh_launch_io_mask(call.dtab(), n, call.grid, invert, lead->stream));   // the plain mask (step 1 of the cleaning is off)
    if (cleaned) {
      const unsigned a = (unsigned)std::min<long>(min_area, 0x7fffffffl);
      HIPCHK(lead, cvh_launch_cc_clean(call.dtab(), n, call.grid, conn, invert, a, fill_holes, keep_largest, lead->stream));
    }
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
    rc = grow(lead, &c->d_contour_edges, &c->contour_edge_cap, E, 0);
    if (rc != CVH_OK) return rc;
    t.dst = c->d_contour_edges;
    t.src_stride = c->contour_edge_cap;
    if (out.loops && out.loops[i]) row_room[(size_t)i] = std::min<size_t>((size_t)out.loop_caps[i], E / 4);
    if (!out.points || !out.points[i]) continue;
    const unsigned long long cap = (unsigned long long)out.point_caps[i];
    point_room[(size_t)i] = (size_t)std::min<unsigned long long>(cap, E);
    if (out.on_host) {
      if (!point_room[(size_t)i]) continue;
      rc = grow(lead, &c->d_contour_points, &c->contour_point_cap, point_room[(size_t)i], 2 * sizeof(int32_t));
      if (rc != CVH_OK) return rc;
      t.src2 = c->d_contour_points;
    } else {
      t.src2 = out.points[i];
    }
    t.h2 = (int)(unsigned)cap; t.w2 = (int)(unsigned)(cap >> 32);
    any_points = true;
  }
  call.grid2 = lay_out(call.tab2, n);
  std::vector<std::vector<cvh_contour_loop>> rows((size_t)n);
  std::vector<std::vector<int32_t>> pts((size_t)n);
  HIPCHK(lead, hipMemcpyAsync((void *)call.dtab2(), call.tab2, (size_t)n * sizeof(CvhIoMember), hipMemcpyHostToDevice, lead->stream));
  HIPCHK(lead, cvh_launch_contours_trace(call.dtab2(), n, call.grid2, conn, simplify, rounds, any_points, lead->stream));
  HIPCHK(lead, hipMemcpyAsync(words, d_words, (size_t)n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, lead->stream));
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    if (row_room[(size_t)i]) {
      rows[(size_t)i].resize(row_room[(size_t)i]);
      HIPCHK(lead, hipMemcpyAsync(rows[(size_t)i].data(), (const uint8_t *)c->d_contour_edges + cvh_contour_rows_offset(c->contour_edge_cap),
                                  row_room[(size_t)i] * sizeof(cvh_contour_loop), hipMemcpyDeviceToHost, lead->stream));
    }
    if (out.on_host && point_room[(size_t)i]) {
      pts[(size_t)i].resize(2 * point_room[(size_t)i]);
      HIPCHK(lead, hipMemcpyAsync(pts[(size_t)i].data(), c->d_contour_points, point_room[(size_t)i] * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, lead->stream));
    }
  }
  rc = close_call(ctxs, n, stream, !out.on_host && any_points);   // (the last read of the pinned block; the caller's stream waits for its points)
  if (rc != CVH_OK) return rc;
  HIPCHK(lead, hipStreamSynchronize(lead->stream));   // the SECOND host wait: counts and rows
  for (int i = 0; i < n; ++i) {
    const size_t L = (size_t)words[4 * i + 1], P = (size_t)words[4 * i + 2];
    if (out.nloops) out.nloops[i] = (long)L;
    if (out.npoints) out.npoints[i] = (long)P;
    if (row_room[(size_t)i]) memcpy(out.loops[i], rows[(size_t)i].data(), std::min(L, row_room[(size_t)i]) * sizeof(cvh_contour_loop));
    if (out.on_host && point_room[(size_t)i]) memcpy(out.points[i], pts[(size_t)i].data(), std::min(P, point_room[(size_t)i]) * 2 * sizeof(int32_t));
  }
  return CVH_OK;
}

int single(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, int simplify, cvh_contour_loop *loops,
           long loop_cap, int32_t *points, long point_cap, long *nloops, long *npoints, void *stream, bool on_host, const char *what)
{
  if (loop_cap < 0) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: loop_cap must not be negative, got %ld", what, loop_cap);
  if (point_cap < 0) return batch_fail(&c, 1, CVH_ERR_ARG, "%s: point_cap must not be negative, got %ld", what, point_cap);
  const Outputs out = {&loops, &loop_cap, &points, &point_cap, nloops, npoints, on_host};
  return contours(&c, 1, conn, invert, min_area, fill_holes, keep_largest, simplify, out, stream, what);
}

}  // namespace

extern "C" int cvh_contours_device_batch(cvh_context *const *ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,
                                         int simplify, cvh_contour_loop *const *loops, const long *loop_caps, int32_t *const *d_points,
                                         const long *point_caps, long *nloops, long *npoints, void *stream)
{
  static const char what[] = "cvh_contours_device_batch";
  const Outputs out = {loops, loop_caps, d_points, point_caps, nloops, npoints, false};
  return guarded(ctxs, n, what, [&]() { return contours(ctxs, n, conn, invert, min_area, fill_holes, keep_largest, simplify, out, stream, what); });
}

extern "C" int cvh_contours_device(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, int simplify,
                                   cvh_contour_loop *loops, long loop_cap, int32_t *d_points, long point_cap, long *nloops, long *npoints,
                                   void *stream)
{
  return guarded_one(c, "cvh_contours_device", [&](const char *what) {
    return single(c, conn, invert, min_area, fill_holes, keep_largest, simplify, loops, loop_cap, d_points, point_cap, nloops, npoints, stream, false, what);
  });
}

extern "C" int cvh_contours(cvh_context *c, int conn, int invert, long min_area, long fill_holes, int keep_largest, int simplify,
                            cvh_contour_loop *loops, long loop_cap, int32_t *points, long point_cap, long *nloops, long *npoints)
{
  return guarded_one(c, "cvh_contours", [&](const char *what) {
    return single(c, conn, invert, min_area, fill_holes, keep_largest, simplify, loops, loop_cap, points, point_cap, nloops, npoints, c->stream, true, what);
  });
}
