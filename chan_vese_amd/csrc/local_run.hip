// local_run.hip — host side of the local-statistics calls (include/chanvese_hip.h, "Local statistics"): plane k of n destination
// contexts becomes the copy, the local mean or the local deviation of a plane of n source contexts.  As colour_run.hip's luma: the
// argument checks (pairs_check: the n destinations followed by the n sources, pair 0's destination leads), then one write_planes
// (cvh_host.h, io_run.hip) around local_kernels.hip's two launches, which leaves the destinations as cvh_set_image of those bytes
// leaves them.  The workspace of the row sums belongs to the destination: a slot per plane it may read, allocated by its first call.
#include "cvh_host.h"

namespace {

// the source planes a pair's MEAN and DEV planes read
int planes_read(const cvh_context *s, const cvh_context *d, const int *what)
{
  unsigned need = 0;
  for (int k = 0; k < d->C; ++k)
    if (what[k] != CVH_LOCAL_COPY) need |= 1u << std::min(k, s->C - 1);
  return __builtin_popcount(need);
}

int local_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, const int *radius, const int *codes, const char *what)
{
  std::vector<cvh_context *> all;
  int rc = pairs_check({srcs, dsts, "srcs", "dsts", "source", "destination", true}, n, what, &all, [&](int i) -> int {
    const cvh_context *s = srcs[i], *d = dsts[i];
    const int *w = codes + (size_t)CVH_MAX_CHANNELS * i;
    if (d->h != s->h || d->w != s->w)
      return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the destination of a %d x %d source must be %d x %d too, got %d x %d", what, i, s->h, s->w,
                        s->h, s->w, d->h, d->w);
    if (radius[i] < 0 || radius[i] > CVH_LOCAL_RADIUS_MAX)
      return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the radius must be 0 .. %d, got %d", what, i, CVH_LOCAL_RADIUS_MAX, radius[i]);
    for (int k = 0; k < d->C; ++k)
      if (w[k] != CVH_LOCAL_COPY && w[k] != CVH_LOCAL_MEAN && w[k] != CVH_LOCAL_DEV)
        return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: what[%d] must be CVH_LOCAL_COPY (0), CVH_LOCAL_MEAN (1) or CVH_LOCAL_DEV (2), got %d", what, i,
                          k, w[k]);
    return CVH_OK;
  }, [&]() -> int {
    if (radius && codes) return CVH_OK;
    return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: the list of %s is NULL", what, radius ? "codes (what)" : "radii");
  });
  if (rc != CVH_OK) return rc;
  rc = pair_sources_have_images(all.data(), n, what, "source");
  if (rc != CVH_OK) return rc;
  bool any_rows = false;
  HIPCHK(all[0], hipSetDevice(all[0]->device));
  for (int i = 0; i < n; ++i) {   // a slot per source plane the destination can read: plane min(k, C_src - 1) for k < C_dst
    if (!planes_read(srcs[i], dsts[i], codes + (size_t)CVH_MAX_CHANNELS * i)) continue;
    any_rows = true;
    cvh_context *d = dsts[i];
    rc = ensure_workspace(d, &d->d_local, (size_t)d->C * cvh_local_slot_bytes(d->h, d->w), "local statistics", false);
    if (rc != CVH_OK) return batch_fail(all.data(), 2 * n, rc, "%s: pair %d: %s", what, i, d->err);
  }
  return write_planes(all.data(), n, 2 * n, what, nullptr, [&](int i, CvhIoMember &m) {
    const cvh_context *s = srcs[i], *d = dsts[i];
    const int *w = codes + (size_t)CVH_MAX_CHANNELS * i;
    m.src = s->d_img_slab;
    m.src_stride = s->img_stride;
    m.w2 = s->C;
    m.h2 = radius[i];
    for (int k = 0; k < d->C; ++k) { m.plane[k] = d->d_img[k]; m.interleaved |= w[k] << (2 * k); }
    m.dst = d->d_local;
    m.nblk = cvh_local_blocks(d->h, d->w, planes_read(s, d, w));
  }, [&](const MemberCall &call) -> int {
    HIPCHK(call.lead, cvh_launch_local(call.dtab(), n, call.grid, any_rows, call.lead->stream));
    ++g_launches[kLocalLaunchSets];
    return CVH_OK;
  });
}

}  // namespace

extern "C" int cvh_local_planes_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, const int *radius, const int *what)
{
  static const char name[] = "cvh_local_planes_batch";
  return guarded(nullptr, 0, name, [&]() { return local_batch(srcs, dsts, n, radius, what, name); });
}

extern "C" int cvh_local_planes(cvh_context *src, cvh_context *dst, int radius, const int *what)
{
  static const char name[] = "cvh_local_planes";
  return guarded(nullptr, 0, name, [&]() { return local_batch(&src, &dst, 1, &radius, what, name); });
}
