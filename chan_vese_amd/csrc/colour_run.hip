// colour_run.hip — host side of the colour-space calls (include/chanvese_hip.h, "Colour spaces"): the three planes of n contexts
// converted in place, or the luma of n three-channel contexts written into n one-channel contexts, in ONE MemberCall (cvh_host.h,
// io_run.hip: member table, stream joins, event ordering) around colour_kernels.hip's launch.  Both end as an ingest does (PlaneSums):
// the contexts whose planes were written are left as cvh_set_image of those bytes leaves them.  The luma call's member list is the n
// destinations followed by the n sources, as pyramid_run.hip's: pair 0's destination leads, the streams of all 2n contexts are joined
// before and after, and the table's first n entries -- the destinations' -- are the kernel's members.
#include "cvh_host.h"

std::atomic<unsigned long> g_colour_launches{0};

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
    if (c->n >= ((size_t)1 << 32))
      return batch_fail(ctxs, n, CVH_ERR_ARG, "%s: member %d: %d x %d is too large, h * w must stay below 2^32", what, i, c->h, c->w);
  }
  for (int i = 0; i < n; ++i)
    if (!ctxs[i]->have_image) return batch_fail(ctxs, n, CVH_ERR_STATE, "%s: member %d has no image (call cvh_set_image first)", what, i);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  rc = settle_all(ctxs, n, what);   // the planes are replaced: iterations in flight are settled, as cvh_set_image does
  if (rc != CVH_OK) return rc;
  PlaneSums back;
  back.plan(ctxs, n);
  MemberCall call;
  rc = call.begin(ctxs, n, what, back.sums_bytes, back.fetch_bytes);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const cvh_context *c = ctxs[i];
    CvhIoMember &m = call.tab[i];
    for (int k = 0; k < 3; ++k) m.plane[k] = c->d_img[k];
    m.sums = back.device_sums(call, i);
    m.nblk = cvh_colour_blocks(c->n);
  }
  rc = call.run(nullptr, false, true, [&]() -> int {   // the ONE host wait of the call: the sums come back to host fields
    HIPCHK(lead, cvh_launch_colour_convert(call.dtab(), n, call.grid, space, order, inverse, lead->stream));
    ++g_colour_launches;
    return back.fetch(call);
  });
  if (rc != CVH_OK) return rc;
  back.arrive(call);
  return CVH_OK;
}

int luma_batch(cvh_context *const *srcs, cvh_context *const *dsts, int n, int order, const char *what)
{
  if (!srcs || !dsts || n < 1)
    return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: empty pair list (srcs = %p, dsts = %p, n = %d)", what, (const void *)srcs, (const void *)dsts, n);
  for (int i = 0; i < n; ++i)
    if (!srcs[i] || !dsts[i]) return batch_fail(nullptr, 0, CVH_ERR_ARG, "%s: pair %d: the %s context is NULL", what, i, srcs[i] ? "destination" : "source");
  std::vector<cvh_context *> all(dsts, dsts + n);
  all.insert(all.end(), srcs, srcs + n);
  cvh_context *const *ctxs = all.data();
  for (int i = 0; i < 2 * n; ++i)
    for (int j = 0; j < i; ++j)
      if (ctxs[i] == ctxs[j])
        return batch_fail(ctxs, 2 * n, CVH_ERR_ARG, "%s: pair %d: its %s context is also pair %d's %s context (a context may be listed once)", what, i % n,
                          i < n ? "destination" : "source", j % n, j < n ? "destination" : "source");
  int rc = order_check(ctxs, 2 * n, order, what);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const cvh_context *s = srcs[i], *d = dsts[i];
    for (const cvh_context *x : {s, d})
      if (x->device != ctxs[0]->device)
        return batch_fail(ctxs, 2 * n, CVH_ERR_ARG, "%s: pair %d: its %s context is on device %d, pair 0's on device %d", what, i,
                          x == s ? "source" : "destination", x->device, ctxs[0]->device);
    if (s->C != 3) return batch_fail(ctxs, 2 * n, CVH_ERR_ARG, "%s: pair %d: the source context has %d channel(s), a luma plane is taken from 3", what, i, s->C);
    if (d->C != 1) return batch_fail(ctxs, 2 * n, CVH_ERR_ARG, "%s: pair %d: the destination context has %d channels, a luma plane goes into 1", what, i, d->C);
    if (d->h != s->h || d->w != s->w)
      return batch_fail(ctxs, 2 * n, CVH_ERR_ARG, "%s: pair %d: the destination of a %d x %d source must be %d x %d too, got %d x %d", what, i, s->h, s->w, s->h,
                        s->w, d->h, d->w);
    if (s->n >= ((size_t)1 << 32))
      return batch_fail(ctxs, 2 * n, CVH_ERR_ARG, "%s: pair %d: %d x %d is too large, h * w must stay below 2^32", what, i, s->h, s->w);
  }
  for (int i = 0; i < n; ++i)
    if (!srcs[i]->have_image) return batch_fail(ctxs, 2 * n, CVH_ERR_STATE, "%s: pair %d: the source context has no image (call cvh_set_image first)", what, i);
  cvh_context *lead = ctxs[0];
  HIPCHK(lead, hipSetDevice(lead->device));
  // the destinations' planes are replaced: their iterations in flight are settled, as cvh_set_image does.  The sources are only read,
  // and no iteration writes planes: theirs stay in flight, ordered before the launch by the stream join
  rc = settle_all(ctxs, n, what);
  if (rc != CVH_OK) return rc;
  PlaneSums back;
  back.plan(ctxs, n);
  MemberCall call;
  rc = call.begin(ctxs, 2 * n, what, back.sums_bytes, back.fetch_bytes);
  if (rc != CVH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const cvh_context *s = srcs[i], *d = dsts[i];
    CvhIoMember &m = call.tab[i];
    m.src = s->d_img_slab;
    m.src_stride = s->img_stride;
    m.plane[0] = d->d_img[0];
    m.sums = back.device_sums(call, i);
    m.nblk = cvh_colour_blocks(d->n);
  }
  rc = call.run(nullptr, false, true, [&]() -> int {   // the ONE host wait of the call: the sums come back to host fields
    HIPCHK(lead, cvh_launch_colour_luma(call.dtab(), n, call.grid, order, lead->stream));
    ++g_colour_launches;
    return back.fetch(call);
  });
  if (rc != CVH_OK) return rc;
  back.arrive(call);
  return CVH_OK;
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
