// window_run.hip — host side of the windowed-plane calls (include/chanvese_hip.h, "Local statistics", "Rank planes" and "Smoothing"): plane k of n
// destination contexts becomes a copy or a windowed filter of plane min(k, C_src - 1) of n source contexts -- the local mean or the
// local deviation; the minimum, the maximum, the median, the opening, the closing or one of the two hats; the blur under a pair's own
// taps or what the blur leaves of the plane.  As colour_run.hip's luma:
// the argument checks (pairs_check: the n destinations followed by the n sources, pair 0's destination leads), then one write_planes
// (cvh_host.h, io_run.hip) around the family's launches (local_kernels.hip, rank_kernels.hip, smooth_kernels.hip), which leaves the destinations as
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
  // optional: a pair's payload (its taps), payload_bytes per pair, which travels beside the member table in the call's one upload and
  // whose device address is the entry's src2.  refuse_payload: CVH_OK, or the refusal of pair i's; fill_payload writes it into `out`.
  size_t payload_bytes = 0;
  const char *payload_name = nullptr;
  int (*refuse_payload)(cvh_context *const *all, int n_all, const char *what, int i, int radius, const void *payload) = nullptr;
  void (*fill_payload)(int radius, const void *payload, void *out) = nullptr;
};

int window_batch(const Family &f, cvh_context *const *srcs, cvh_context *const *dsts, int n, const int *radius, const int *codes, const char *what,
                 const void *const *payloads = nullptr)
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
    return f.payload_bytes ? f.refuse_payload(all.data(), 2 * n, what, i, radius[i], payloads[i]) : CVH_OK;
  }, [&]() -> int {
    if (radius && codes && (payloads || !f.payload_bytes)) return CVH_OK;
    return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: the list of %s is NULL", what, !radius ? "radii" : !codes ? "codes (what)" : f.payload_name);
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
  }, f.payload_bytes, [&](int i, void *out) { f.fill_payload(radius[i], payloads[i], out); });
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

// smoothing: the one pass beside the writer's is the row pass, for the source planes a pair's BLUR and DETAIL planes read; the payload is
// the pair's taps, R + 1 of them padded with zeros to CVH_SMOOTH_TAPS
Plan smooth_plan(const cvh_context *s, const cvh_context *d, int radius, const int *what)
{
  unsigned need = 0;
  for (int k = 0; k < d->C; ++k)
    if (what[k] != CVH_SMOOTH_COPY) need |= 1u << std::min(k, s->C - 1);
  return Plan{need ? 1u : 0u, cvh_smooth_blocks(d->h, d->w, radius, __builtin_popcount(need))};
}

int smooth_refuse_code(cvh_context *const *all, int n_all, const char *what, int i, int k, int code)
{
  return code == CVH_SMOOTH_COPY || code == CVH_SMOOTH_BLUR || code == CVH_SMOOTH_DETAIL ? CVH_OK
       : batch_fail(all, n_all, CVH_ERR_ARG, "%s: pair %d: what[%d] must be CVH_SMOOTH_COPY (0), CVH_SMOOTH_BLUR (1) or CVH_SMOOTH_DETAIL (2), got %d", what, i, k, code);
}

int smooth_refuse_taps(cvh_context *const *all, int n_all, const char *what, int i, int radius, const void *payload)
{
  const uint16_t *t = (const uint16_t *)payload;
  if (!t) return batch_fail(all, n_all, CVH_ERR_ARG, "%s: pair %d: its list of taps is NULL", what, i);
  long sum = t[0];
  for (int j = 1; j <= radius; ++j) sum += 2l * t[j];
  return sum == CVH_SMOOTH_TAP_SUM ? CVH_OK
       : batch_fail(all, n_all, CVH_ERR_ARG, "%s: pair %d: taps[0] + 2 (taps[1] + .. + taps[%d]) must be %d, got %ld", what, i, radius, CVH_SMOOTH_TAP_SUM, sum);
}

void smooth_fill_taps(int radius, const void *payload, void *out)
{
  memset(out, 0, CVH_SMOOTH_TAPS * sizeof(uint16_t));
  memcpy(out, payload, (size_t)(radius + 1) * sizeof(uint16_t));
}

const Family kSmooth = {
    /* refuse_code */ smooth_refuse_code, /* median, median_radius_max */ -1, 0, /* radius_max */ CVH_SMOOTH_RADIUS_MAX, /* bits */ 2,
    /* workspace */ &cvh_context::d_smooth, /* slot_bytes */ cvh_smooth_slot_bytes, /* slots */ 1, /* workspace_name */ "smoothing",
    /* plan */ smooth_plan, /* launch */ cvh_launch_smooth, /* counter */ kSmoothLaunchSets,
    /* payload_bytes, payload_name */ CVH_SMOOTH_TAPS * sizeof(uint16_t), "tap lists",
    /* refuse_payload */ smooth_refuse_taps, /* fill_payload */ smooth_fill_taps};

}  // namespace

extern "C" int cvh_smooth_planes_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, const int *radius, const uint16_t *const *taps, const int *what)
{
  static const char name[] = "cvh_smooth_planes_batch";
  return guarded(nullptr, 0, name, [&]() { return window_batch(kSmooth, srcs, dsts, n, radius, what, name, (const void *const *)taps); });
}

extern "C" int cvh_smooth_planes(cvh_context *src, cvh_context *dst, int radius, const uint16_t *taps, const int *what)
{
  static const char name[] = "cvh_smooth_planes";
  return guarded(nullptr, 0, name, [&]() { return window_batch(kSmooth, &src, &dst, 1, &radius, what, name, (const void *const *)&taps); });
}

// THE Gaussian of the library (include/chanvese_hip.h, "Smoothing"): host only, no context; the message of a refusal is cvh_last_error(NULL)'s
extern "C" int cvh_gauss_taps(double sigma, uint16_t *taps, int *radius)
{
  if (!taps || !radius) return fail(nullptr, CVH_ERR_ARG, "cvh_gauss_taps: %s is NULL", taps ? "radius" : "taps");
  if (!std::isfinite(sigma) || sigma <= 0.0 || sigma > 21.0)
    return fail(nullptr, CVH_ERR_ARG, "cvh_gauss_taps: sigma must be finite and in (0, 21], got %g", sigma);
  const int R = (int)ceil(3.0 * sigma);
  double e[CVH_SMOOTH_TAPS], S = 1.0;
  e[0] = 1.0;
  for (int i = 1; i <= R; ++i) { e[i] = exp(-((double)i * (double)i) / (2.0 * sigma * sigma)); S += 2.0 * e[i]; }
  long rest = CVH_SMOOTH_TAP_SUM;
  memset(taps, 0, CVH_SMOOTH_TAPS * sizeof(uint16_t));
  for (int i = 1; i <= R; ++i) { taps[i] = (uint16_t)floor(32768.0 * e[i] / S + 0.5); rest -= 2l * taps[i]; }
  taps[0] = (uint16_t)rest;
  *radius = R;
  return CVH_OK;
}

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
