// init_run.hip — host side of the device-side initial level sets (include/chanvese_hip.h, "Device-side initial level sets"): the grey
// histogram, Otsu's threshold and the threshold / rectangle / disk starts of n contexts, each ONE MemberCall (cvh_host.h, io_run.hip:
// member table, stream joins, event ordering) around init_kernels.hip's launches.  The single-context calls are batches of one member
// (guarded_one); what the members must hold is asked of csv_batch.hip's predicates.  The histogram calls only read the planes; a start
// is a level set arriving without crossing to the host, as cvh_init_checkerboard_batch's.
#include "cvh_host.h"

namespace {

inline int bins_of(const cvh_context *c) { return 255 * c->C + 1; }

// x as a double, rounded to nearest even (what Python's float(int) does).  The top 64 bits convert with one rounding at bit 11; the bits
// shifted out only matter as "something is set below", which the lowest kept bit can carry: it lies below the rounding position.
double to_double_rne(unsigned __int128 x)
{
  const unsigned long long hi = (unsigned long long)(x >> 64);
  if (!hi) return (double)(unsigned long long)x;
  const int shift = 64 - __builtin_clzll(hi);
  unsigned long long m = (unsigned long long)(x >> shift);
  if (x & ((((unsigned __int128)1) << shift) - 1)) m |= 1;
  return ldexp((double)m, shift);
}

// the header's definition, word for word
int otsu(const uint32_t *hist, int bins, int *t)
{
  unsigned long long N = 0, S = 0;   // bins <= 766: N < 2^42, S < 2^52
  int v0 = -1;
  for (int v = 0; v < bins; ++v) {
    N += hist[v]; S += (unsigned long long)v * hist[v];
    if (hist[v] && v0 < 0) v0 = v;
  }
  if (!N) return CVH_ERR_ARG;
  unsigned long long n0 = 0, s0 = 0;
  double best = -1.0;
  int arg = v0;   // a single occupied bin has no candidate
  for (int v = 0; v + 1 < bins; ++v) {
    n0 += hist[v]; s0 += (unsigned long long)v * hist[v];
    if (!n0 || n0 >= N) continue;
    const __int128 d = (__int128)S * n0 - (__int128)N * s0;
    const unsigned __int128 q = (unsigned __int128)n0 * (N - n0);
    const double fd = to_double_rne((unsigned __int128)(d < 0 ? -d : d));   // (the sign leaves with the square)
    const double score = (fd * fd) / to_double_rne(q);
    if (score > best) { best = score; arg = v; }
  }
  *t = arg;
  return CVH_OK;
}

// what every call checks before anything is touched: the list, and planes the 32-bit counters and pixel indices cover
int members_fit(cvh_context *const *ctxs, int n, const char *what)
{
  const int rc = members_check(ctxs, n, what, kMembersListed);
  return rc != CVH_OK ? rc : members_below(ctxs, n, what, 32);
}

// The histograms of n members (checked by the caller): iterations in flight settled, the counters zeroed, ONE launch, the counters
// fetched into the leader's pinned block, ONE host wait.  Afterwards member i's 255 C_i + 1 counts are at h_io + (*off)[i], until the
// next call that stages.
int histograms(cvh_context *const *ctxs, int n, std::vector<size_t> *off, const char *what)
{
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  int rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  size_t host_bytes = 0;
  off->assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    cvh_context *c = ctxs[i];
    rc = ensure_workspace(c, (void **)&c->d_hist, (size_t)bins_of(c) * sizeof(unsigned), "histogram", false);
    if (rc != CVH_OK) return batch_fail(ctxs, n, rc, "%s: member %d: %s", what, i, c->err);
    (*off)[i] = host_bytes;
    host_bytes += align_up((size_t)bins_of(c) * sizeof(unsigned), 256);
  }
  MemberCall call;
  rc = call.begin(ctxs, n, what, 0, host_bytes);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    CvhIoMember &m = call.tab[i];
    for (int k = 0; k < c->C; ++k) m.plane[k] = c->d_img[k];
    m.sums = (unsigned long long *)c->d_hist;
    m.nblk = cvh_io_blocks(c->n);
    (*off)[i] += call.host_off;
  }
  return call.run(nullptr, false, true, [&]() -> int {   // the ONE host wait: the counts
    for (int i = 0; i < n; ++i) HIPCHK(lead, hipMemsetAsync(ctxs[i]->d_hist, 0, (size_t)bins_of(ctxs[i]) * sizeof(unsigned), lead->stream));
    HIPCHK(lead, cvh_launch_init_histogram(call.dtab(), n, call.grid, lead->stream));
    for (int i = 0; i < n; ++i)
      HIPCHK(lead, hipMemcpyAsync(call.hb + (*off)[i], ctxs[i]->d_hist, (size_t)bins_of(ctxs[i]) * sizeof(unsigned), hipMemcpyDeviceToHost, lead->stream));
    return CVH_OK;
  });
}

// The starts par[0 .. n-1] of n members (checked by the caller, iterations in flight settled): ONE launch writes every level set into the
// buffer cvh_set_levelset writes and does the device's half of a new run; behind the wait every member begins that run.
int starts(cvh_context *const *ctxs, int n, const CvhInitStart *par, const char *what)
{
  cvh_context *lead = ctxs[0];
  MemberCall call;
  int rc = call.begin(ctxs, n, what, (size_t)n * sizeof(CvhInitStart));
  if (rc != CVH_OK) return rc;
  memcpy(call.hb + call.extra_off, par, (size_t)n * sizeof(CvhInitStart));
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    CvhIoMember &m = call.tab[i];
    for (int k = 0; k < c->C; ++k) m.plane[k] = c->d_img[k];
    levelset_target(c, &m);
    m.nblk = cvh_init_start_blocks(c->n);
  }
  const CvhInitStart *d_par = (const CvhInitStart *)(call.db + call.extra_off);
  rc = call.run(nullptr, false, true, [&]() -> int { HIPCHK(lead, cvh_launch_init_start(call.dtab(), d_par, n, call.grid, lead->stream)); return CVH_OK; });
  return rc != CVH_OK ? rc : call.arrived();
}

// a start that needs no histogram: settle, then launch
int settled_starts(cvh_context *const *ctxs, int n, const CvhInitStart *par, const char *what)
{
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  const int rc = settle_all(ctxs, n, what);
  return rc != CVH_OK ? rc : starts(ctxs, n, par, what);
}

CvhInitStart start_of(int mode, double inside, double outside, long long a, long long b, long long c, long long d)
{
  CvhInitStart s;
  memset(&s, 0, sizeof(s));
  s.inside = inside; s.outside = outside; s.a = a; s.b = b; s.c = c; s.d = d; s.mode = mode;
  return s;
}

int histogram_batch(cvh_context *const *ctxs, int n, uint32_t *const *hists, const int *caps, int *bins, const char *what)
{
  int rc = members_fit(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (!hists || !caps) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of host buffers or of their capacities is NULL", what);
  for (int i = 0; i < n; ++i) {
    if (caps[i] < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: cap must not be negative, got %d", what, i, caps[i]);
    if (caps[i] > 0 && !hists[i]) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: the host buffer is NULL", what, i);
  }
  rc = members_have_images(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  std::vector<size_t> off;
  rc = histograms(ctxs, n, &off, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const int B = bins_of(ctxs[i]);
    if (caps[i] > 0) memcpy(hists[i], (const unsigned char *)ctxs[0]->h_io + off[i], (size_t)std::min(B, caps[i]) * sizeof(uint32_t));
  }
  if (bins) *bins = bins_of(ctxs[0]);
  return CVH_OK;
}

// t[i] = Otsu's threshold of member i (t may be null); with start, the threshold start behind it
int otsu_batch(cvh_context *const *ctxs, int n, int *t, bool start, double inside, double outside, const char *what)
{
  int rc = members_fit(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  rc = members_have_images(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  std::vector<size_t> off;
  rc = histograms(ctxs, n, &off, what);
  if (rc != CVH_OK) return rc;
  std::vector<int> ts((size_t)n, 0);
  for (int i = 0; i < n; ++i) {   // (an empty histogram behind a launch that ran is the device's failure, not the caller's: CVH_ERR_HIP)
    rc = otsu((const uint32_t *)((const unsigned char *)ctxs[0]->h_io + off[i]), bins_of(ctxs[i]), &ts[i]);
    if (rc != CVH_OK) return batch_fail(ctxs, n, CVH_ERR_HIP, "%s: member %d: the device counted no pixel", what, i);
    if (t) t[i] = ts[i];
  }
  if (!start) return CVH_OK;
  std::vector<CvhInitStart> par;
  for (int i = 0; i < n; ++i) par.push_back(start_of(CVH_START_THRESHOLD, inside, outside, ts[i], 0, 0, 0));
  return starts(ctxs, n, par.data(), what);
}

int threshold_batch(cvh_context *const *ctxs, int n, const int *t, double inside, double outside, const char *what)
{
  int rc = members_fit(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (!t) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of thresholds is NULL", what);
  std::vector<CvhInitStart> par;
  for (int i = 0; i < n; ++i) {
    if (t[i] < 0 || t[i] >= bins_of(ctxs[i]))
      return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: t must be in 0 .. %d, got %d", what, i, bins_of(ctxs[i]) - 1, t[i]);
    par.push_back(start_of(CVH_START_THRESHOLD, inside, outside, t[i], 0, 0, 0));
  }
  rc = members_have_images(ctxs, n, what);
  return rc != CVH_OK ? rc : settled_starts(ctxs, n, par.data(), what);
}

int rect_batch(cvh_context *const *ctxs, int n, const int *xywh, double inside, double outside, const char *what)
{
  const int rc = members_fit(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (!xywh) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of rectangles is NULL", what);
  std::vector<CvhInitStart> par;
  for (int i = 0; i < n; ++i) {
    const long long x = xywh[4 * i], y = xywh[4 * i + 1], rw = xywh[4 * i + 2], rh = xywh[4 * i + 3];
    if (rw <= 0 || rh <= 0)
      return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: the rectangle's width and height must be positive, got %lld x %lld", what, i, rw, rh);
    // clipped to the plane; an empty intersection (x1 <= x0 or y1 <= y0) holds no pixel
    par.push_back(start_of(CVH_START_RECT, inside, outside, std::max(x, 0LL), std::min<long long>(x + rw, ctxs[i]->w), std::max(y, 0LL),
                           std::min<long long>(y + rh, ctxs[i]->h)));
  }
  return settled_starts(ctxs, n, par.data(), what);
}

int disk_batch(cvh_context *const *ctxs, int n, const int *cxcyr, double inside, double outside, const char *what)
{
  const int rc = members_fit(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  if (!cxcyr) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: the list of disks is NULL", what);
  std::vector<CvhInitStart> par;
  for (int i = 0; i < n; ++i) {
    if (cxcyr[3 * i + 2] < 0) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: the radius must not be negative, got %d", what, i, cxcyr[3 * i + 2]);
    par.push_back(start_of(CVH_START_DISK, inside, outside, cxcyr[3 * i], cxcyr[3 * i + 1], cxcyr[3 * i + 2], 0));
  }
  return settled_starts(ctxs, n, par.data(), what);
}

}  // namespace

extern "C" int cvh_otsu_from_histogram(const uint32_t *hist, int bins, int *t)
{
  if (!hist || !t) return fail(nullptr, CVH_ERR_ARG, "cvh_otsu_from_histogram: hist or t is NULL");
  if (bins < 1 || bins > CVH_HIST_MAX_BINS) return fail(nullptr, CVH_ERR_ARG, "cvh_otsu_from_histogram: bins must be in 1 .. %d, got %d", CVH_HIST_MAX_BINS, bins);
  if (otsu(hist, bins, t) != CVH_OK) return fail(nullptr, CVH_ERR_ARG, "cvh_otsu_from_histogram: the histogram is empty");
  return CVH_OK;
}

extern "C" int cvh_histogram_batch(cvh_context *const *ctxs, int n, uint32_t *const *hists, const int *caps)
{
  static const char what[] = "cvh_histogram_batch";
  return guarded(ctxs, n, what, [&]() { return histogram_batch(ctxs, n, hists, caps, nullptr, what); });
}

extern "C" int cvh_histogram(cvh_context *c, uint32_t *hist, int cap, int *bins)
{
  return guarded_one(c, "cvh_histogram", [&](const char *what) { return histogram_batch(&c, 1, &hist, &cap, bins, what); });
}

extern "C" int cvh_otsu_threshold(cvh_context *c, int *t)
{
  return guarded_one(c, "cvh_otsu_threshold", [&](const char *what) {
    return t ? otsu_batch(&c, 1, t, false, 0.0, 0.0, what) : fail(c, CVH_ERR_ARG, "%s: t is NULL", what);
  });
}

extern "C" int cvh_init_otsu_batch(cvh_context *const *ctxs, int n, int *t, double inside, double outside)
{
  static const char what[] = "cvh_init_otsu_batch";
  return guarded(ctxs, n, what, [&]() { return otsu_batch(ctxs, n, t, true, inside, outside, what); });
}

extern "C" int cvh_init_otsu(cvh_context *c, int *t, double inside, double outside)
{
  return guarded_one(c, "cvh_init_otsu", [&](const char *what) { return otsu_batch(&c, 1, t, true, inside, outside, what); });
}

extern "C" int cvh_init_threshold_batch(cvh_context *const *ctxs, int n, const int *t, double inside, double outside)
{
  static const char what[] = "cvh_init_threshold_batch";
  return guarded(ctxs, n, what, [&]() { return threshold_batch(ctxs, n, t, inside, outside, what); });
}

extern "C" int cvh_init_threshold(cvh_context *c, int t, double inside, double outside)
{
  return guarded_one(c, "cvh_init_threshold", [&](const char *what) { return threshold_batch(&c, 1, &t, inside, outside, what); });
}

extern "C" int cvh_init_rect_batch(cvh_context *const *ctxs, int n, const int *xywh, double inside, double outside)
{
  static const char what[] = "cvh_init_rect_batch";
  return guarded(ctxs, n, what, [&]() { return rect_batch(ctxs, n, xywh, inside, outside, what); });
}

extern "C" int cvh_init_rect(cvh_context *c, int x, int y, int rw, int rh, double inside, double outside)
{
  const int xywh[4] = {x, y, rw, rh};
  return guarded_one(c, "cvh_init_rect", [&](const char *what) { return rect_batch(&c, 1, xywh, inside, outside, what); });
}

extern "C" int cvh_init_disk_batch(cvh_context *const *ctxs, int n, const int *cxcyr, double inside, double outside)
{
  static const char what[] = "cvh_init_disk_batch";
  return guarded(ctxs, n, what, [&]() { return disk_batch(ctxs, n, cxcyr, inside, outside, what); });
}

extern "C" int cvh_init_disk(cvh_context *c, int cx, int cy, int r, double inside, double outside)
{
  const int cxcyr[3] = {cx, cy, r};
  return guarded_one(c, "cvh_init_disk", [&](const char *what) { return disk_batch(&c, 1, cxcyr, inside, outside, what); });
}
