// window_run.hip — host side of the windowed-plane calls (include/chanvese_hip.h, "Local statistics" and "Rank planes"): plane k of n
// destination contexts becomes a copy or a windowed filter of plane min(k, C_src - 1) of n source contexts -- the local mean or the
// local deviation; the minimum, the maximum, the median, the opening, the closing or one of the two hats.  As colour_run.hip's luma:
// the argument checks (pairs_check: the n destinations followed by the n sources, pair 0's destination leads), then one write_planes
// (cvh_host.h, io_run.hip) around the family's launches (local_kernels.hip, rank_kernels.hip), which leaves the destinations as
// cvh_set_image of those bytes leaves them.  A family's workspace belongs to the destination, allocated by its first call that needs it.
#include "cvh_host.h"
#include "rank_math.h"

namespace {

// window_batch is the one sequence, a Family says what differs.  A pair's Plan: which passes run (0: the writer's alone, no workspace), its workgroups
struct Plan { unsigned passes, nblk; };

struct Family {
  int (*refuse_code)(cvh_context *const *all, int n_all, const char *what, int i, int k, int code);   // CVH_OK, or the refusal of what[k]
  int median, median_radius_max;     // the code whose radius is bound to median_radius_max (-1: none)
  int radius_max, bits;              // radii 0 .. radius_max; bits per code in CvhIoMember::interleaved
  void *cvh_context::*workspace;     // the destination's workspace: `slots` times slot_bytes per plane of the destination; its name
  size_t (*slot_bytes)(int h, int w);
  int slots; const char *workspace_name;
  Plan (*plan)(const cvh_context *s, const cvh_context *d, int radius, const int *what);
  hipError_t (*launch)(const CvhIoMember *tab, int nmem, unsigned grid, unsigned passes, hipStream_t s);   // passes: every pair's, ORed
  LaunchCounter counter;
};

int window_batch(const Family &f, cvh_context *const *srcs, cvh_context *const *dsts, int n, const int *radius, const int *codes, const char *what)
{
  std::vector<cvh_context *> all;
  int rc = pairs_check({srcs, dsts, "srcs", "dsts", "source", "destination", true}, n, what, &all, [&](int i) -> int {
    const cvh_context *s = srcs[i], *d = dsts[i];
    const int *w = codes + (size_t)CVH_MAX_CHANNELS * i;
    if (d->h != s->h || d->w != s->w)
      return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the destination of a %d x %d source must be %d x %d too, got %d x %d", what, i, s->h, s->w,
                        s->h, s->w, d->h, d->w);
    if (radius[i] < 0 || radius[i] > f.radius_max)
      return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the radius must be 0 .. %d, got %d", what, i, f.radius_max, radius[i]);
    for (int k = 0; k < d->C; ++k) {
      if (const int refused = f.refuse_code(all.data(), 2 * n, what, i, k, w[k])) return refused;
      if (w[k] == f.median && radius[i] > f.median_radius_max)
        return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the radius of a median (what[%d]) must be 0 .. %d, got %d", what, i, k,
                          f.median_radius_max, radius[i]);
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
  for (int i = 0; i < n; ++i) {   // room for every source plane the destination can read: plane min(k, C_src - 1) for k < C_dst
    const Plan p = f.plan(srcs[i], dsts[i], radius[i], codes + (size_t)CVH_MAX_CHANNELS * i);
    if (!p.passes) continue;
    passes |= p.passes;
    cvh_context *d = dsts[i];
    rc = ensure_workspace(d, &(d->*f.workspace), (size_t)d->C * f.slots * f.slot_bytes(d->h, d->w), f.workspace_name, false);
    if (rc != CVH_OK) return batch_fail(all.data(), 2 * n, rc, "%s: pair %d: %s", what, i, d->err);
  }
  return write_planes(all.data(), n, 2 * n, what, nullptr, [&](int i, CvhIoMember &m) {
    const cvh_context *s = srcs[i], *d = dsts[i];
    const int *w = codes + (size_t)CVH_MAX_CHANNELS * i;
    m.src = s->d_img_slab;
    m.src_stride = s->img_stride;
    m.w2 = s->C;
    m.h2 = radius[i];
    for (int k = 0; k < d->C; ++k) { m.plane[k] = d->d_img[k]; m.interleaved |= w[k] << (f.bits * k); }
    m.dst = d->*f.workspace;
    m.nblk = f.plan(s, d, radius[i], w).nblk;
  }, [&](const MemberCall &call) -> int {
    HIPCHK(call.lead, f.launch(call.dtab(), n, call.grid, passes, call.lead->stream));
    ++g_launches[f.counter];
    return CVH_OK;
  });
}

// local statistics: the one pass beside the writer's is the row pass, for the source planes a pair's MEAN and DEV planes read
Plan local_plan(const cvh_context *s, const cvh_context *d, int, const int *what)
{
  unsigned need = 0;
  for (int k = 0; k < d->C; ++k)
    if (what[k] != CVH_LOCAL_COPY) need |= 1u << std::min(k, s->C - 1);
  return Plan{need ? 1u : 0u, cvh_local_blocks(d->h, d->w, __builtin_popcount(need))};
}

int local_refuse_code(cvh_context *const *all, int n_all, const char *what, int i, int k, int code)
{
  return code == CVH_LOCAL_COPY || code == CVH_LOCAL_MEAN || code == CVH_LOCAL_DEV ? CVH_OK
       : batch_fail(all, n_all, CVH_ERR_ARG, "%s: pair %d: what[%d] must be CVH_LOCAL_COPY (0), CVH_LOCAL_MEAN (1) or CVH_LOCAL_DEV (2), got %d", what, i, k, code);
}

const Family kLocal = {
    /* refuse_code */ local_refuse_code, /* median, median_radius_max */ -1, 0, /* radius_max */ CVH_LOCAL_RADIUS_MAX, /* bits */ 2,
    /* workspace */ &cvh_context::d_local, /* slot_bytes */ cvh_local_slot_bytes, /* slots */ 1, /* workspace_name */ "local statistics",
    /* plan */ local_plan, /* launch */ cvh_launch_local, /* counter */ kLocalLaunchSets};

// rank planes: the chains whose row pass runs, whether one of them runs twice, the source planes of the median
Plan rank_plan(const cvh_context *s, const cvh_context *d, int radius, const int *what)
{
  unsigned chains = 0, medians = 0, passes = 0;
  for (int k = 0; k < d->C; ++k) {
    const int from = std::min(k, s->C - 1), chain = cvh_rank_chain(what[k]);
    if (chain >= 0) {
      chains |= 1u << (2 * from + chain);
      passes |= CVH_RANK_PASS_ROWS | (cvh_rank_twice(what[k]) ? CVH_RANK_PASS_TWICE : 0u);
    } else if (what[k] == CVH_RANK_MEDIAN && radius > 0) {
      medians |= 1u << from;
      passes |= CVH_RANK_PASS_MEDIAN;
    }
  }
  return Plan{passes, cvh_rank_blocks(d->h, d->w, radius, __builtin_popcount(chains), __builtin_popcount(medians))};
}

int rank_refuse_code(cvh_context *const *all, int n_all, const char *what, int i, int k, int code)
{
  return code >= CVH_RANK_COPY && code <= CVH_RANK_BOTHAT ? CVH_OK
       : batch_fail(all, n_all, CVH_ERR_ARG, "%s: pair %d: what[%d] must be one of CVH_RANK_COPY (0) .. CVH_RANK_BOTHAT (7), got %d", what, i, k, code);
}

const Family kRank = {
    /* refuse_code */ rank_refuse_code, /* median, median_radius_max */ CVH_RANK_MEDIAN, CVH_RANK_MEDIAN_RADIUS_MAX, /* radius_max */ CVH_RANK_RADIUS_MAX,
    /* bits */ 3, /* workspace */ &cvh_context::d_rank, /* slot_bytes */ cvh_rank_slot_bytes, /* slots */ CVH_RANK_SLOTS,
    /* workspace_name */ "rank planes", /* plan */ rank_plan, /* launch */ cvh_launch_rank, /* counter */ kRankLaunchSets};

}  // namespace

extern "C" int cvh_local_planes_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, const int *radius, const int *what)
{
  static const char name[] = "cvh_local_planes_batch";
  return guarded(nullptr, 0, name, [&]() { return window_batch(kLocal, srcs, dsts, n, radius, what, name); });
}

extern "C" int cvh_local_planes(cvh_context *src, cvh_context *dst, int radius, const int *what)
{
  static const char name[] = "cvh_local_planes";
  return guarded(nullptr, 0, name, [&]() { return window_batch(kLocal, &src, &dst, 1, &radius, what, name); });
}

extern "C" int cvh_rank_planes_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, const int *radius, const int *what)
{
  static const char name[] = "cvh_rank_planes_batch";
  return guarded(nullptr, 0, name, [&]() { return window_batch(kRank, srcs, dsts, n, radius, what, name); });
}

extern "C" int cvh_rank_planes(cvh_context *src, cvh_context *dst, int radius, const int *what)
{
  static const char name[] = "cvh_rank_planes";
  return guarded(nullptr, 0, name, [&]() { return window_batch(kRank, &src, &dst, 1, &radius, what, name); });
}
