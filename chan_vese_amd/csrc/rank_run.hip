// rank_run.hip — host side of the rank-plane calls (include/chanvese_hip.h, "Rank planes"): plane k of n destination contexts becomes
// the copy, the minimum, the maximum, the median, the opening, the closing or one of the two hats of a plane of n source contexts.  As
// local_run.hip: the argument checks (pairs_check: the n destinations followed by the n sources, pair 0's destination leads), then one
// write_planes (cvh_host.h, io_run.hip) around rank_kernels.hip's launches, which leaves the destinations as cvh_set_image of those bytes
// leaves them.  The workspace of the byte planes between the passes belongs to the destination, allocated by its first call.
#include "cvh_host.h"
#include "rank_math.h"

namespace {

// what a pair asks of the kernels: the chains whose row pass runs, whether one of them runs twice, the source planes of the median
struct Plan { int row_jobs = 0, median_planes = 0; unsigned passes = 0; };

Plan plan_of(const cvh_context *s, const cvh_context *d, int radius, const int *what)
{
  unsigned chains = 0, medians = 0;
  Plan p;
  for (int k = 0; k < d->C; ++k) {
    const int from = std::min(k, s->C - 1), chain = cvh_rank_chain(what[k]);
    if (chain >= 0) {
      chains |= 1u << (2 * from + chain);
      p.passes |= CVH_RANK_PASS_ROWS | (cvh_rank_twice(what[k]) ? CVH_RANK_PASS_TWICE : 0u);
    } else if (what[k] == CVH_RANK_MEDIAN && radius > 0) {
      medians |= 1u << from;
      p.passes |= CVH_RANK_PASS_MEDIAN;
    }
  }
  p.row_jobs = __builtin_popcount(chains);
  p.median_planes = __builtin_popcount(medians);
  return p;
}

int rank_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, const int *radius, const int *codes, const char *what)
{
  std::vector<cvh_context *> all;
  int rc = pairs_check({srcs, dsts, "srcs", "dsts", "source", "destination", true}, n, what, &all, [&](int i) -> int {
    const cvh_context *s = srcs[i], *d = dsts[i];
    const int *w = codes + (size_t)CVH_MAX_CHANNELS * i;
    if (d->h != s->h || d->w != s->w)
      return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the destination of a %d x %d source must be %d x %d too, got %d x %d", what, i, s->h, s->w,
                        s->h, s->w, d->h, d->w);
    if (radius[i] < 0 || radius[i] > CVH_RANK_RADIUS_MAX)
      return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the radius must be 0 .. %d, got %d", what, i, CVH_RANK_RADIUS_MAX, radius[i]);
    for (int k = 0; k < d->C; ++k) {
      if (w[k] < CVH_RANK_COPY || w[k] > CVH_RANK_BOTHAT)
        return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: what[%d] must be one of CVH_RANK_COPY (0) .. CVH_RANK_BOTHAT (7), got %d", what, i, k, w[k]);
      if (w[k] == CVH_RANK_MEDIAN && radius[i] > CVH_RANK_MEDIAN_RADIUS_MAX)
        return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the radius of a median (what[%d]) must be 0 .. %d, got %d", what, i, k,
                          CVH_RANK_MEDIAN_RADIUS_MAX, radius[i]);
    }
    return CVH_OK;
  }, [&]() -> int {
    if (radius && codes) return CVH_OK;
    return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: the list of %s is NULL", what, radius ? "codes (what)" : "radii");
  });
  if (rc != CVH_OK) return rc;
  rc = pair_sources_have_images(all.data(), n, what, "source");
  if (rc != CVH_OK) return rc;
  unsigned passes = 0;
  HIPCHK(all[0], hipSetDevice(all[0]->device));
  for (int i = 0; i < n; ++i) {   // CVH_RANK_SLOTS byte planes per source plane the destination can read: plane min(k, C_src - 1) for k < C_dst
    const Plan p = plan_of(srcs[i], dsts[i], radius[i], codes + (size_t)CVH_MAX_CHANNELS * i);
    if (!p.passes) continue;
    passes |= p.passes;
    cvh_context *d = dsts[i];
    rc = ensure_workspace(d, &d->d_rank, (size_t)d->C * CVH_RANK_SLOTS * cvh_rank_slot_bytes(d->h, d->w), "rank planes", false);
    if (rc != CVH_OK) return batch_fail(all.data(), 2 * n, rc, "%s: pair %d: %s", what, i, d->err);
  }
  return write_planes(all.data(), n, 2 * n, what, nullptr, [&](int i, CvhIoMember &m) {
    const cvh_context *s = srcs[i], *d = dsts[i];
    const int *w = codes + (size_t)CVH_MAX_CHANNELS * i;
    const Plan p = plan_of(s, d, radius[i], w);
    m.src = s->d_img_slab;
    m.src_stride = s->img_stride;
    m.w2 = s->C;
    m.h2 = radius[i];
    for (int k = 0; k < d->C; ++k) { m.plane[k] = d->d_img[k]; m.interleaved |= w[k] << (3 * k); }
    m.dst = d->d_rank;
    m.nblk = cvh_rank_blocks(d->h, d->w, radius[i], p.row_jobs, p.median_planes);
  }, [&](const MemberCall &call) -> int {
    HIPCHK(call.lead, cvh_launch_rank(call.dtab(), n, call.grid, passes, call.lead->stream));
    ++g_launches[kRankLaunchSets];
    return CVH_OK;
  });
}

}  // namespace

extern "C" int cvh_rank_planes_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, const int *radius, const int *what)
{
  static const char name[] = "cvh_rank_planes_batch";
  return guarded(nullptr, 0, name, [&]() { return rank_batch(srcs, dsts, n, radius, what, name); });
}

extern "C" int cvh_rank_planes(cvh_context *src, cvh_context *dst, int radius, const int *what)
{
  static const char name[] = "cvh_rank_planes";
  return guarded(nullptr, 0, name, [&]() { return rank_batch(&src, &dst, 1, &radius, what, name); });
}
