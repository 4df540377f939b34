// pyramid_run.hip — host side of the coarse-to-fine calls (include/chanvese_hip.h, "Coarse-to-fine"): the planes of fine contexts
// restricted into coarse ones, the level sets of coarse contexts prolonged into fine ones, n pairs in ONE MemberCall (cvh_host.h,
// io_run.hip: member table, stream joins, event ordering) around pyramid_kernels.hip's launch.  The call's member list is pairs_check's
// (csv_batch.hip), the n destinations followed by the n sources: pair 0's destination leads (its stream carries the launch), the
// streams of all 2n contexts are joined before and after, and the table's first n entries -- the destinations' -- are the kernel's
// members.  A restrict is its checks, then one write_planes (io_run.hip: it ends as an ingest does); a prolong ends as a device-side
// start does (levelset_target, MemberCall::arrived).
#include "cvh_host.h"

namespace {

// What every call checks for every pair before anything is touched.  all = [dst 0 .. n-1, src 0 .. n-1] is filled here.
int pyramid_pairs(cvh_context *const *fines, cvh_context *const *coarses, int n, bool down, const char *what, std::vector<cvh_context *> *all)
{
  return pairs_check({fines, coarses, "fines", "coarses", "fine", "coarse", down}, n, what, all, [&](int i) -> int {
    const cvh_context *f = fines[i], *c = coarses[i];
    if (f->C != c->C)
      return batch_fail(all->data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the fine context has %d channel(s), the coarse one %d", what, i, f->C, c->C);
    if (c->h != (f->h + 1) / 2 || c->w != (f->w + 1) / 2)
      return batch_fail(all->data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the coarse context of a %d x %d plane must be %d x %d, got %d x %d", what, i, f->h, f->w,
                        (f->h + 1) / 2, (f->w + 1) / 2, c->h, c->w);
    return CVH_OK;
  });
}

int restrict_batch(cvh_context *const *fines, cvh_context *const *coarses, int n, const char *what)
{
  std::vector<cvh_context *> all;
  int rc = pyramid_pairs(fines, coarses, n, true, what, &all);
  if (rc != CVH_OK) return rc;
  rc = pair_sources_have_images(all.data(), n, what, "fine");
  if (rc != CVH_OK) return rc;
  return write_planes(all.data(), n, 2 * n, what, nullptr, [&](int i, CvhIoMember &m) {
    const cvh_context *c = coarses[i], *f = fines[i];
    m.src = f->d_img_slab;
    m.src_stride = f->img_stride;
    m.h2 = f->h; m.w2 = f->w;
    for (int k = 0; k < c->C; ++k) m.plane[k] = c->d_img[k];
    m.nblk = cvh_restrict_blocks(f->h, f->w);
  }, [&](const MemberCall &call) -> int {
    HIPCHK(call.lead, cvh_launch_restrict(call.dtab(), n, call.grid, call.lead->stream));
    ++g_launches[kPyramidLaunches];
    return CVH_OK;
  });
}

int prolong_batch(cvh_context *const *coarses, cvh_context *const *fines, int n, const char *what)
{
  std::vector<cvh_context *> all;
  int rc = pyramid_pairs(fines, coarses, n, false, what, &all);
  if (rc != CVH_OK) return rc;
  cvh_context *const *ctxs = all.data();
  for (int i = 0; i < n; ++i)
    if (!coarses[i]->have_u) return batch_fail(ctxs, 2 * n, CVH_ERR_STATE, "%s: pair %d: the coarse context has no level set", what, i);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  rc = settle_all(ctxs, 2 * n, what);   // the fine level sets are replaced, the coarse ones read as the getters read them
  if (rc != CVH_OK) return rc;
  rc = members_mirrors_fresh(ctxs, 2 * n, what, n, "pair");   // (the coarse contexts are members n .. 2n-1)
  if (rc != CVH_OK) return rc;
  MemberCall call;
  rc = call.begin(ctxs, 2 * n, what);
  if (rc != CVH_OK) return rc;
  std::vector<int> is_fine((size_t)2 * n, 0);
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = coarses[i];
    CvhIoMember &m = call.tab[i];   // (h, w: the fine grid)
    m.src = c->d_u[current_buffer(c)];
    levelset_target(fines[i], &m);
    m.nblk = cvh_prolong_blocks(fines[i]->h, fines[i]->w);
    is_fine[i] = 1;
  }
  rc = call.run(nullptr, false, true, [&]() -> int {
    HIPCHK(lead, cvh_launch_prolong(call.dtab(), n, call.grid, lead->stream));
    ++g_launches[kPyramidLaunches];
    return CVH_OK;
  });
  return rc != CVH_OK ? rc : call.arrived(is_fine.data());
}

}  // namespace

extern "C" int cvh_restrict_image_batch(cvh_context *const *fines, cvh_context *const *coarses, int n)
{
  static const char what[] = "cvh_restrict_image_batch";
  return guarded(nullptr, 0, what, [&]() { return restrict_batch(fines, coarses, n, what); });
}

extern "C" int cvh_restrict_image(cvh_context *fine, cvh_context *coarse)
{
  static const char what[] = "cvh_restrict_image";
  return guarded(nullptr, 0, what, [&]() { return restrict_batch(&fine, &coarse, 1, what); });
}

extern "C" int cvh_prolong_levelset_batch(cvh_context *const *coarses, cvh_context *const *fines, int n)
{
  static const char what[] = "cvh_prolong_levelset_batch";
  return guarded(nullptr, 0, what, [&]() { return prolong_batch(coarses, fines, n, what); });
}

extern "C" int cvh_prolong_levelset(cvh_context *coarse, cvh_context *fine)
{
  static const char what[] = "cvh_prolong_levelset";
  return guarded(nullptr, 0, what, [&]() { return prolong_batch(&coarse, &fine, 1, what); });
}
