// colour_run.hip — host side of the colour-space calls (include/chanvese_hip.h, "Colour spaces"): the three planes of n contexts
// converted in place, or the luma of n three-channel contexts written into n one-channel contexts.  Each call is its own argument
// checks, then one write_planes (cvh_host.h, io_run.hip) around colour_kernels.hip's launch: the contexts whose planes were written are
// left as cvh_set_image of those bytes leaves them.  The luma call's member list is pairs_check's (csv_batch.hip): the n destinations
// followed by the n sources; pair 0's destination leads, and the table's first n entries -- the destinations' -- are the kernel's members.
#include "cvh_host.h"

namespace {

int order_check(cvh_context *const *ctxs, int n, int order, const char *what)
{
  if (order == CVH_ORDER_BGR || order == CVH_ORDER_RGB) return CVH_OK;
  return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: order must be CVH_ORDER_BGR (0) or CVH_ORDER_RGB (1), got %d", what, order);
}

int convert_batch(cvh_context *const *ctxs, int n, int space, int order, int inverse, const char *what)
{
  int rc = members_check(ctxs, n, what, kMembersListed);
  if (rc != CVH_OK) return rc;
  if (space != CVH_COLOUR_YCRCB && space != CVH_COLOUR_YUV)
    return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: space must be CVH_COLOUR_YCRCB (1) or CVH_COLOUR_YUV (2), got %d", what, space);
  rc = order_check(ctxs, n, order, what);
  if (rc != CVH_OK) return rc;
  if (inverse != 0 && inverse != 1) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: inverse must be 0 or 1, got %d", what, inverse);
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    if (c->C != 3) return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d has %d channel(s), a colour conversion takes 3", what, i, c->C);
    rc = members_below(ctxs, n, what, 32, i);
    if (rc != CVH_OK) return rc;
  }
  rc = members_have_images(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  return write_planes(ctxs, n, n, what, nullptr, [&](int i, CvhIoMember &m) {
    for (int k = 0; k < 3; ++k) m.plane[k] = ctxs[i]->d_img[k];
    m.nblk = cvh_colour_blocks(ctxs[i]->n);
  }, [&](const MemberCall &call) -> int {
    HIPCHK(call.lead, cvh_launch_colour_convert(call.dtab(), n, call.grid, space, order, inverse, call.lead->stream));
    ++g_launches[kColourLaunches];
    return CVH_OK;
  });
}

int luma_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, int order, const char *what)
{
  std::vector<cvh_context *> all;
  int rc = pairs_check({srcs, dsts, "srcs", "dsts", "source", "destination", true}, n, what, &all, [&](int i) -> int {
    const cvh_context *s = srcs[i], *d = dsts[i];
    if (s->C != 3) return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the source context has %d channel(s), a luma plane is taken from 3", what, i, s->C);
    if (d->C != 1) return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the destination context has %d channels, a luma plane goes into 1", what, i, d->C);
    if (d->h != s->h || d->w != s->w)
      return batch_fail(all.data(), 2 * n, CVH_ERR_ARG, "%s: pair %d: the destination of a %d x %d source must be %d x %d too, got %d x %d", what, i, s->h, s->w,
                        s->h, s->w, d->h, d->w);
    return CVH_OK;
  }, [&]() { return order_check(all.data(), 2 * n, order, what); });
  if (rc != CVH_OK) return rc;
  rc = pair_sources_have_images(all.data(), n, what, "source");
  if (rc != CVH_OK) return rc;
  return write_planes(all.data(), n, 2 * n, what, nullptr, [&](int i, CvhIoMember &m) {
    m.src = srcs[i]->d_img_slab;
    m.src_stride = srcs[i]->img_stride;
    m.plane[0] = dsts[i]->d_img[0];
    m.nblk = cvh_colour_blocks(dsts[i]->n);
  }, [&](const MemberCall &call) -> int {
    HIPCHK(call.lead, cvh_launch_colour_luma(call.dtab(), n, call.grid, order, call.lead->stream));
    ++g_launches[kColourLaunches];
    return CVH_OK;
  });
}

}  // namespace

extern "C" int cvh_convert_colour_batch(cvh_context *const *ctxs, int n, int space, int order, int inverse)
{
  static const char what[] = "cvh_convert_colour_batch";
  return guarded(nullptr, 0, what, [&]() { return convert_batch(ctxs, n, space, order, inverse, what); });
}

extern "C" int cvh_convert_colour(cvh_context *ctx, int space, int order, int inverse)
{
  static const char what[] = "cvh_convert_colour";
  return guarded(nullptr, 0, what, [&]() { return convert_batch(&ctx, 1, space, order, inverse, what); });
}

extern "C" int cvh_luma_image_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, int order)
{
  static const char what[] = "cvh_luma_image_batch";
  return guarded(nullptr, 0, what, [&]() { return luma_batch(srcs, dsts, n, order, what); });
}

extern "C" int cvh_luma_image(cvh_context *src, cvh_context *dst, int order)
{
  static const char what[] = "cvh_luma_image";
  return guarded(nullptr, 0, what, [&]() { return luma_batch(&src, &dst, 1, order, what); });
}
